#!/usr/bin/env python3
"""bench.py -- headline benchmark of the MI355X-native dense contrastive segmentation hot path.

    python bench.py --gpus N --steps K --warmup W [--config 2|4] [--workload step|loss] [--full] [--dump-outputs DIR]

N > 1 is launched by the driver through torch.distributed.run (one rank per GPU, RCCL).  Rank 0
prints ONE JSON line.  `value` is the whole-job rate; the timed region is bracketed by a barrier and
torch.cuda.synchronize() on both sides and the maximum over ranks is taken.  `ms_per_step` is the time of one of the K
timed steps.

A plain run sets up, runs the W warm-up and K timed steps and prints the line.  Everything else it measures --
`contrastive_loss_fwd_bwd_ms` of the step workload, `roofline*`, `cpu_baseline`, the plain-config and eager comparator
timings, --kernel-table -- runs only under --full.  --dump-outputs DIR writes what the last timed step computed as
DIR/<name>.npy (step: loss and its terms, logits, the projection heads' embeddings, metrics, the updated parameters and
buffers; loss workload: loss and feature gradients), larger arrays as a fixed seeded sample; the inputs depend on the
arguments only, so two builds can be compared output for output.

Workloads:
  step  (default) one training step of BASELINE.json configs[1] -- HRNet-W48 + LossWrapper(CE + 0.1 * DCV2_ms, 3 scales
        + cross-scale), synthetic Cityscapes 512x1024, batch 12 per GPU -- exactly the body of
        BaseManager.train_one_epoch on a resident batch: forward, loss, backward, SGD, LR schedule AND the per-step
        metrics tail of the reference (confusion matrix, pixel accuracies, mIoU, logging; HRNet_Manager.py:117-121).
        `--config 4`: UPerNet + Swin-T, ADE20K 512x512, TwoScaleLoss + DCV2_ms (4 scales), AdamW, batch 16 per GPU.
  loss  the contrastive loss alone (forward + backward) on synthetic 256-d projector outputs
Extra keys of the JSON line (--full):
  roofline                    step: the kernel SYMBOL with the largest share of one step (all its launches, every shape), time-
        weighted: sum of the launches' algorithmic FLOPs / sum of their HIP-event durations, measured live in ONE extra step
        after the timed region with events on the launch streams (mscs_amd/utils/kernel_timer.py); loss workload: the InfoNCE
        backward sweep.  `traffic` only where a PMC pass of that kernel is committed (else null)
  roofline_other              the other matrix-pipe symbols of that step (same accounting), the head's 144 -> 720 weight gradient
        and forward launches alone, the InfoNCE backward sweep alone
  roofline_hbm                the streaming kernels of that step against the 8 TB/s HBM peak: K1 label_hist, K2 rank_select, K3
        gather_normalize, K6 normalize_bwd_scatter and the batch-norm kernels -- algorithmic bytes / event time
  cpu_baseline                oracle/eager_torch.py + the same model code on the host cores, every part MEASURED on the full
        workload (no multiplication): the model's forward + backward + SGD over all `batch` images (in micro-batches of 4:
        host memory) and one evaluation of the whole contrastive loss (every scale and cross-scale term)
  plain_config_ms_per_step    the same step with explicit `false` for graph.lazy_logits / lazy_projector and train.fused_optimizer
        (the headline config holds the reference's keys only; this package's managers choose the fused consumers themselves)
  eager_gpu_step_ms, speedup_vs_eager_gpu_step   the reference-structure eager step on the same GPU in the same run
        (stock MIOpen / ATen kernels + the eager-structure loss of oracle/eager_torch.py): BASELINE.json's >= 5x target
  contrastive_loss_fwd_bwd_ms, metrics_in_step, peak_mem_gb
`dtype` "f32 (f16x3-emulated)": fp32 storage and accumulation everywhere; the matrix products of the loss and of every
3x3 convolution run as three split-f16 (hi, lo) MFMA passes whose results match fp32 to round-off (DESIGN.md section
3); `--mfma f32`, `--branch-conv library` and graph key head_conv='library' select plain f32 MFMA / MIOpen instead.
"""
import argparse
import contextlib
import ctypes
import json
import os
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MFMA_F32_PEAK_TFLOPS = 157.3      # /opt/skills/guides/MI355X_MICROARCH.md, "Peak FP32 (matrix)"
MFMA_F16_PEAK_TFLOPS = 2500.0     # same guide, "Peak BF16/FP16 MFMA ~2.5 PF dense"
# f16x3 backward sweep: both products (S recompute and H.B, 2NMC algorithmic FLOP each) are issued as 3 f16 MFMA
# passes (hi.hi + hi.lo + lo.hi), so the matrix-pipe roofline for the 4NMC algorithmic FLOP is 2500 / 3 TFLOP/s.
MFMA_F16X3_BWD_PEAK_TFLOPS = MFMA_F16_PEAK_TFLOPS / 3.0


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default=None, choices=["step", "loss"])
    ap.add_argument("--config", type=int, default=2, choices=[2, 4, 5],
                    help="BASELINE.json configs[] index of the timed workload: 2 = HRNet-W48 Cityscapes 512x1024 (the "
                         "headline metric, default), 4 = UPerNet + Swin-T ADE20K 512x512 with per-GPU batch 16 "
                         "(SURVEY.md Appendix C case 4': the whole global batch of configs[3] on one GPU), 5 = UPerNet + "
                         "Swin-L 640x640 + cross-scale contrastive (configs[4]) with per-GPU batch 16")
    ap.add_argument("--batch", type=int, default=None, help="per-GPU batch (weak scaling); default 12 / 16 by config")
    ap.add_argument("--height", type=int, default=None)
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--scales", type=int, default=None)
    ap.add_argument("--no-cross", action="store_true")
    ap.add_argument("--labels", choices=["iid", "blocky"], default="iid",
                    help="iid: uniform per pixel, the worst case that pins N at the 10 000 cap (the headline); blocky: uniform at "
                         "1/32 resolution, repeated 32 x 32 (SURVEY section 8d: the realistic-layout check)")
    ap.add_argument("--mfma", default=None, choices=["f32", "f16x3"],
                    help="similarity-product arithmetic of the loss kernels (default: the library default)")
    ap.add_argument("--branch-conv", default="f16x3", choices=["f16x3", "library"],
                    help="backbone 3x3 convolutions: direct split-f16 kernel (fp32-equivalent) or MIOpen f32")
    ap.add_argument("--conv1x1", default="f16x3", choices=["f16x3", "gemm", "library"],
                    help="1x1 convolutions: f16x3 kernels (weight gradient always, forward / data gradient below 64 MB)"
                         " | batched fp32 library GEMMs | MIOpen")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--amp", action="store_true", help="bf16 autocast for the model (loss stays fp32)")
    ap.add_argument("--channels-last", action="store_true")
    ap.add_argument("--miopen-benchmark", action="store_true",
                    help="cudnn.benchmark=True like the reference (BaseManager.py:122). OFF by default: on a fresh box "
                         "MIOpen's exhaustive fp32 solver search for HRNet-W48's ~300 conv shapes takes > 20 minutes")
    ap.add_argument("--no-eager-miopen-benchmark", dest="eager_miopen_benchmark", action="store_false",
                    help="do not time the eager-structure comparator a second time with torch.backends.cudnn.benchmark "
                         "= True (the reference's setting, BaseManager.py:122).  On this image the solver search of the "
                         "warm-up step takes ~4 s (profiles/r03_bench_miopen_find.json), so both ratios are printed by "
                         "default")
    ap.add_argument("--eager-baseline", action="store_true",
                    help="also time the eager-structure restatement of the loss alone on the GPU")
    ap.add_argument("--no-eager-step", action="store_true",
                    help="skip eager_gpu_step_ms (the eager-structure reference step on the same GPU, N=1 only)")
    ap.add_argument("--materialize-logits", action="store_true",
                    help="HRNet returns the up-sampled logits like the reference instead of the lazy 1/4-resolution form "
                         "(graph key lazy_logits) that the fused up-sampling + cross-entropy kernels consume")
    ap.add_argument("--materialize-projector", action="store_true",
                    help="the projection heads return their full [n, d, h, w] maps like the reference instead of the lazy form "
                         "(graph key lazy_projector) whose last 1x1 convolution the loss evaluates on the sampled pixels only")
    ap.add_argument("--feature-layout", choices=["nchw", "nhwc"], default="nchw",
                    help="loss workload: memory layout of the synthetic embedding maps (nhwc = channels-last strides, what "
                         "this package's projector hands out in training; nchw = a plain contiguous map)")
    ap.add_argument("--detail-file", default=None,
                    help="write the FULL record (per-shape tables, roofline_other / roofline_hbm, notes) to this JSON file; it always "
                         "goes to stderr as one 'bench-detail: {...}' line.  stdout carries the compact line only (<= 4 KB)")
    ap.add_argument("--kernel-table", default=None,
                    help="write the in-step per-kernel table (the rows behind `roofline*`) to this JSON file")
    ap.add_argument("--no-reference-config", action="store_true",
                    help="skip the second timing with lazy_logits / lazy_projector / fused optimizer off")
    ap.add_argument("--plain-config", action="store_true",
                    help="time the step with this repo's opt-in graph / train keys off (what a reference JSON config gives)")
    ap.add_argument("--no-metrics", action="store_true",
                    help="leave the per-step metrics tail (confusion matrix, accuracies, mIoU, logging) out of the step")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: roofline / per-kernel figures, contrastive_loss_fwd_bwd_ms, the CPU "
                         "baseline, the plain-config and eager comparator timings.  Off: set up, warm up, time the steps, "
                         "(--dump-outputs) and print the line")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (float32 / float64, "
                         "a fixed seeded sample of the larger arrays, <= 64 MB in all)")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    for flag, given in (("--kernel-table", a.kernel_table), ("--eager-baseline", a.eager_baseline)):
        if given and not a.full:
            ap.error(f"{flag} is a --full measurement")
    d = {2: (12, 512, 1024, 3), 4: (16, 512, 512, 4), 5: (16, 640, 640, 4)}[a.config]
    a.batch = a.batch or d[0]
    a.height = a.height or d[1]
    a.width = a.width or d[2]
    a.scales = a.scales or d[3]
    a.classes = 20 if a.config == 2 else 151
    a.dataset = "CITYSCAPES" if a.config == 2 else "ADE20K"
    return a


MFMA_MODE = None


def loss_config(S, cross, dataset="CITYSCAPES"):
    weights = [1.0, 0.7, 0.4, 0.1][:S]
    extra = {"mfma_mode": MFMA_MODE} if MFMA_MODE else {}
    return {**extra, "dataset": dataset, "experiment": 1, "temperature": 0.1, "scales": S,
            "weights": weights, "cross_scale_contrast": cross, "min_views_per_class": 5,
            "max_views_per_class": 2500, "max_features_total": 10000, "label_scaling_mode": "nn"}


def synth_labels(args, n, H, W, gen):
    """int64 [n, H, W]: iid-uniform classes (worst-case load: every class in every image, N at the cap), or "blocky":
    uniform at 1/32 resolution, each value repeated over a 32 x 32 block (class regions as in real masks)."""
    K = getattr(args, "classes", 20)
    if getattr(args, "labels", "iid") == "blocky":
        small = torch.randint(0, K, (n, (H + 31) // 32, (W + 31) // 32), generator=gen)
        return small.repeat_interleave(32, 1).repeat_interleave(32, 2)[:, :H, :W].contiguous()
    return torch.randint(0, K, (n, H, W), generator=gen)


def synth_loss_inputs(args, dev, rank):
    gen = torch.Generator().manual_seed(1000 * rank)
    n, H, W = args.batch, args.height, args.width
    label = synth_labels(args, n, H, W, gen).to(dev)
    fmt = torch.channels_last if getattr(args, "feature_layout", "nchw") == "nhwc" else torch.contiguous_format
    feats = [torch.randn(n, 256, H // (4 << s), W // (4 << s), generator=gen).to(dev).contiguous(memory_format=fmt)
             .requires_grad_(True) for s in range(args.scales)]
    return label, feats


def time_loss_only(args, dev, rank, world):
    import mscs_amd  # noqa: F401
    from mscs_amd.losses import DenseContrastiveLossV2_ms
    from mscs_amd.utils import set_verbosity
    set_verbosity(40)
    cross = not args.no_cross
    mod = DenseContrastiveLossV2_ms(loss_config(args.scales, cross, getattr(args, "dataset", "CITYSCAPES")))
    label, feats = synth_loss_inputs(args, dev, rank)
    torch.manual_seed(0)

    def step():
        for f in feats:
            f.grad = None
        loss = mod(label, feats)
        loss.backward()
        return loss

    for _ in range(args.warmup):
        step()
    sync(world)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    sync(world)
    dt = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        # what a caller of the loss receives: its value and the gradients of the feature maps
        arrays = {"loss": loss.detach().double().reshape(1)}
        arrays.update({f"grad_s{s}": f.grad for s, f in enumerate(feats)})
        dump_outputs(args.dump_outputs, arrays)
    return dt, mod


DUMP_SAMPLE = 1 << 20        # elements kept of a larger output: a fixed, seeded sample (4 MB in float32)
DUMP_PIXELS = 4096           # pixel positions kept of an embedding map (all of its channels)
DUMP_LIMIT = 64 << 20


def _seed_of(name):
    import zlib
    return zlib.crc32(name.encode())


def _flat_sample(name, t):
    """t flattened; above DUMP_SAMPLE elements, the elements at DUMP_SAMPLE sorted positions drawn from a generator seeded
    by the array's name (same shape -> same positions in every run and every build)."""
    import numpy as np
    flat = t.detach().reshape(-1)
    if flat.numel() <= DUMP_SAMPLE:
        return flat
    idx = np.sort(np.random.default_rng(_seed_of(name)).integers(0, flat.numel(), DUMP_SAMPLE))
    return flat[torch.from_numpy(idx).to(flat.device)]


def _embedding_sample(name, f):
    """[DUMP_PIXELS, d]: the embedding at fixed, seeded (image, pixel) positions of an [n, d, h, w] map -- or of the lazy
    projection (models/Projector.LazyProjection) that stands for it, evaluated at those pixels only."""
    import numpy as np
    n, d, h, w = f.shape
    rng = np.random.default_rng(_seed_of(name))
    b = torch.from_numpy(rng.integers(0, n, DUMP_PIXELS)).to(f.device)
    pix = torch.from_numpy(rng.integers(0, h * w, DUMP_PIXELS)).to(f.device)
    if hasattr(f, "rows"):
        return f.rows(b.int(), pix.int().view(-1, 1))
    return f.detach().reshape(n, d, h * w)[b, :, pix]


def dump_outputs(out_dir, arrays):
    """name -> tensor: DIR/<name>.npy, float64 for float64 tensors and float32 otherwise, larger arrays sampled."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    total = 0
    with torch.no_grad():
        for name, t in arrays.items():
            if t is None:
                continue
            t = _flat_sample(name, t) if t.numel() > DUMP_SAMPLE else t.detach()
            a = t.cpu().numpy().astype(np.float64 if t.dtype == torch.float64 else np.float32)
            total += a.nbytes
            if total > DUMP_LIMIT:
                raise RuntimeError(f"--dump-outputs: more than {DUMP_LIMIT >> 20} MB at {name}")
            np.save(os.path.join(out_dir, name + ".npy"), a)
    print(f"bench: {len(os.listdir(out_dir))} outputs in {out_dir} ({total / 2 ** 20:.1f} MB)", file=sys.stderr, flush=True)


def step_outputs(mgr, ret, args):
    """What the caller of one training step receives -- the loss and its terms, the logits, the projection heads' embeddings,
    the step's metrics -- and what the step leaves in the model: its parameters and floating-point buffers after the update.
    Lazy outputs are evaluated the way a consumer would (UpsampledLogits.materialize(), LazyProjection at sampled pixels)."""
    def dense(x):
        return x.materialize() if hasattr(x, "materialize") and not hasattr(x, "rows") else x

    arrays = {"loss": ret["loss"].detach().double().reshape(1)}
    for k, v in getattr(mgr.loss, "loss_vals", {}).items():
        if torch.is_tensor(v):
            arrays[f"loss_{k}"] = v.detach().double().reshape(1)
    arrays["logits"] = _flat_sample("logits", dense(ret["output"]))
    if ret.get("interm_output") is not None:
        arrays["interm_logits"] = _flat_sample("interm_logits", dense(ret["interm_output"]))
    for s, f in enumerate(ret.get("feats") or []):
        arrays[f"embedding_s{s}"] = _embedding_sample(f"embedding_s{s}", f)
    if not args.no_metrics:
        arrays["metrics"] = torch.tensor([mgr.metrics[k] for k in ("pa", "pac", "miou")], dtype=torch.float64)
    arrays["params"] = _flat_sample("params", torch.cat([p.detach().reshape(-1) for p in mgr.model.parameters()]))
    bufs = [b.detach().reshape(-1) for b in mgr.model.buffers() if b.is_floating_point()]
    if bufs:
        arrays["buffers"] = _flat_sample("buffers", torch.cat(bufs))
    return arrays


def sync(world):
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
        torch.cuda.synchronize()


def _time_launches(launch, iters):
    launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def roofline_conv_kernels(args, dev, iters=20):
    """Average launch duration of the step's dominant hand-written kernels, HIP events on the launch stream.

    Since round 3 the head convolution runs over the branch maps (ops.conv3x3_over_upsampled): what is left of it at full
    resolution is a 144 -> 720 convolution.  The kernel family with the largest share of a step is the weight gradient
    `k_wgrad3x3d<3,1>` (17 % of the kernel time, profiles/r03_step_kernels.csv); its heaviest launch is that head part
    (batch x 144 -> 720 x H/4 x W/4), which is what `roofline` reports (kernel + its slab reduction).  `roofline_other`:
    the forward / data-gradient kernel `k_conv3x3_il<3,4>` on the same layer, the 48-channel BasicBlock shape
    (`k_conv3x3_il_ws2<1,4>` and its weight gradient) and the InfoNCE backward sweep.
    Algorithmic FLOPs = 2 * N * Cout * Cin * 9 * H * W; every one of them costs three f16 MFMA passes
    (hi.hi + hi.lo + lo.hi), hence peak = 2500 / 3 TFLOP/s."""
    from mscs_amd.models import ops
    from mscs_amd.models.amax import amax_of
    n, h, w = args.batch, args.height // 4, args.width // 4
    gen = torch.Generator(device=dev).manual_seed(1)
    peak = MFMA_F16_PEAK_TFLOPS / 3.0
    note = "every algorithmic FLOP is issued as 3 f16 MFMA passes (split-f16, fp32-equivalent): 2.5 PFLOP/s / 3"

    def entry(kernel, flops, ms, abytes, pmc=None):
        # pmc = (FETCH_SIZE, WRITE_SIZE) KiB per launch of a committed rocprofv3 --pmc pass on exactly this kernel and shape
        e = {"bound": "mfma", "kernel": kernel, "achieved": round(flops / (ms * 1e-3) / 1e12, 2), "peak": round(peak, 1),
             "unit": "TFLOP/s", "frac": round(flops / (ms * 1e-3) / 1e12 / peak, 4), "peak_note": note, "traffic": None,
             "traffic_source": "not collected for this kernel / shape (profiles/r03_conv_pmc_*.csv hold the per-kernel "
                               "FETCH_SIZE / WRITE_SIZE of tools/per_shape_roofline.py)",
             "algorithmic_bytes": abytes, "launch_ms": round(ms, 4)}
        if pmc:
            e["traffic"] = (2 * pmc[0] + pmc[1]) * 1024
            e["traffic_source"] = ("constant from profiles/r03_head_wgrad_pmc.csv (separate rocprofv3 --pmc passes of "
                                   "tools/probes/head_wgrad_pmc.sh, not read live; 2 x FETCH_SIZE + WRITE_SIZE = bytes that "
                                   "crossed L2 <-> fabric, Infinity-Cache hits included)")
        return e

    def conv_and_wgrad(ci, co, it):
        x = torch.randn(n, ci, h, w, device=dev, generator=gen).relu_()
        wt = torch.randn(co, ci, 3, 3, device=dev, generator=gen) * (2.0 / (9 * ci)) ** 0.5
        gy = torch.randn(n, co, h, w, device=dev, generator=gen) * 1e-4
        xa, wa = amax_of(x), amax_of(wt)
        amax_of(gy)
        wp = ops.conv3x3_pack(wt, wa)
        out = torch.empty(n, co, h, w, device=dev)
        flops = 2.0 * n * co * ci * 9 * h * w
        ms_f = _time_launches(lambda: ops.conv3x3_launch(x, wp, co, xa, wa, out), it)
        ms_w = _time_launches(lambda: ops.conv3x3_wgrad(x, gy), it)
        return flops, ms_f, ms_w, (n * (ci + co) * h * w) * 4

    flops, ms_f, ms_w, ab = conv_and_wgrad(144, 720, 8)
    main = entry(f"k_wgrad3x3d<3,1,wave-level splits> + k_wgrad_reduce (dcl_wgrad3x3_f16x3): 3x3 weight gradient, "
                 f"{n}x(144->720)x{h}x{w} (the head convolution's full-resolution part; 135 tile pairs x 7 pixel splits on "
                 "1024 waves)", flops, ms_w, ab, PMC_HEAD_WGRAD if (n, h, w) == (12, 128, 256) else None)
    others = [entry(f"k_conv3x3_il<3,4> (dcl_conv3x3_f16x3): 3x3 conv forward, {n}x(144->720)x{h}x{w}", flops, ms_f, ab,
                    PMC_HEAD_FWD if (n, h, w) == (12, 128, 256) else None)]
    torch.cuda.empty_cache()
    flops, ms_f, ms_w, ab = conv_and_wgrad(48, 48, iters)
    others.append(entry(f"k_conv3x3_il_ws2<1,4> (dcl_conv3x3_f16x3): 3x3 conv forward / data gradient, {n}x48x{h}x{w}",
                        flops, ms_f, ab))
    others.append(entry(f"k_wgrad3x3d<3,1> + k_wgrad_reduce (dcl_wgrad3x3_f16x3), {n}x48x{h}x{w}", flops, ms_w, ab))
    return main, others


# HBM-side bytes per launch from committed rocprofv3 --pmc passes of the step (tools/pmc_step.sh -> profiles/r04_step_pmc.csv),
# (FETCH_SIZE KiB, WRITE_SIZE KiB) averaged over the symbol's launches of one step; traffic = (2 * FETCH + WRITE) KiB per the gfx950
# correction of MI355X_MICROARCH.md.  Keys = kernel symbols of mscs_amd/utils/kernel_timer.py.
PMC_STEP = {
    "k_wgrad3x3d<3,1,false>": (92674.1, 6739.6),        # (+ k_wgrad_reduce_t: 3.5 MiB fetched per launch)
    "k_wgrad3x3d_pre<3,1,false>": (90401.9, 6733.6),    # (round 6: the x operand is the raw tensor in front of the norm)
    "k_wgrad3x3d<3,1,true>": (577186.6, 25996.2),       # (13 launches since round 6, the head's 144 -> 720 one among them)
    "k_conv3x3_il_ws2<1,4>": (50397.9, 77759.8),
    "k_conv3x3_il_ws2_pre<1,4>": (39808.2, 76458.7),
    "k_conv3x3_il<3,4>": (35729.6, 46166.0),
    "k_conv3x3_il_pre<3,4>": (17849.4, 31795.2),
    "k_conv3x3_il<3,2>": (27364.8, 9216.0),
    "k_conv3x3_il_pre<3,2>": (25828.0, 9216.0),
    "k_conv3x3_pm<2,1>": (16443.0, 76595.3),
    "k_conv3x3_il_s2<3>": (35150.1, 22656.0),
    "k_conv3x3_il_s2<2>": (38106.8, 18432.0),
    "k_wgrad3x3_s2d<3,1>": (78111.8, 6564.9),
    "k_bn_bwd_apply<true>": (46739.8, 70047.6),
    "k_bn_bwd_reduce<true>": (46585.2, 13.0),
    "k_bn_apply<true,true>": (49305.7, 50777.2),
    "k_bn_apply<true,false>": (35200.7, 70116.0),       # (9 launches left: transitions, the stem's bn2, layer 1's bn2)
    "k_bn_stats": (24204.5, 18.7),
    "k_bn_stats_pre": (20792.3, 223.8),
    "k_bn_bwd_apply<false>": (20456.9, 24197.0),
    "k_bn_bwd_reduce<false>": (20339.8, 12.8),
    "k_bn_apply<false,false>": (11414.2, 22639.7),
    "k_upsample_fwd": (37566.5, 64049.4),
    "k_upsample_bwd_rows": (63130.8, 9767.5),
    "k_sweep<MODE_Z>": (104674.5, 21132.7),             # (since it keeps the positives' similarities: 21 MB written per launch)
    "k_sweep<MODE_BWD,stream-K>": (60576.3, 71687.9),
    "k_gather_normalize": (88214.8, 19796.6),           # K3 on the lazily projected rows (round 6: the two HBM legs of the loss
    "k_normalize_bwd_scatter": (51025.5, 52123.4),      # that had no constant here; the counters were in the csv all along)
    "k_head_norm_dz": (644087.4, 1106016.0),
}
PMC_STEP_SOURCE = "profiles/r06_step_pmc_fetch.csv, r06_step_pmc_write.csv"


def roofline_from_rows(rows, args):
    """`roofline` = the matrix-pipe kernel SYMBOL with the largest share of one step, time-weighted over all its launches
    (sum of algorithmic FLOPs / sum of HIP-event durations); `roofline_other` = the next symbols; `roofline_hbm` = the
    streaming kernels (K1 / K2 / K3 / K6 and the batch-norm family) against the HBM peak.  One extra, SERIALISED step after the
    timed region (every launch on one stream, so an event pair holds one kernel: mscs_amd/utils/kernel_timer.py)."""
    total_ms = sum(r["total_ms"] for r in rows)

    def entry(r):
        top = sorted(r["shapes"].items(), key=lambda kv: -kv[1][1])[:4]
        e = {"bound": r["bound"], "kernel": f"{r['kernel']} ({r['entry']}): all {r['calls']} launches of one training step "
                                            f"(serialised replay), time-weighted",
             "achieved": round(r["achieved"], 2), "peak": round(r["peak"], 1), "unit": r["unit"], "frac": round(r["frac"], 4),
             "launches": r["calls"], "launch_ms": round(r["total_ms"] / r["calls"], 4), "step_ms": round(r["total_ms"], 3),
             "share_of_timed_kernels": round(r["total_ms"] / total_ms, 4),
             "algorithmic_flops" if r["bound"] == "mfma" else "algorithmic_bytes":
                 (r["flops"] if r["bound"] == "mfma" else r["bytes"]) / r["calls"],
             "shapes": [{"shape": k, "launches": v[0], "avg_ms": round(v[1] / v[0], 4),
                         "frac": round(((v[2] / 1e12 if r["bound"] == "mfma" else v[3] / 1e9) / (v[1] / v[0] * 1e-3)) / r["peak"], 4)}
                        for k, v in top],
             "traffic": None, "traffic_source": "no PMC pass committed for this symbol"}
        if r["bound"] == "mfma":
            e["peak_note"] = "every algorithmic FLOP is issued as 3 f16 MFMA passes (split-f16, fp32-equivalent): 2.5 PFLOP/s / 3"
        pmc = PMC_STEP.get(r["kernel"])
        if pmc and (args.batch, args.height, args.width) == (12, 512, 1024):
            e["traffic"] = (2 * pmc[0] + pmc[1]) * 1024
            e["traffic_source"] = (f"constant from {PMC_STEP_SOURCE} (separate rocprofv3 --pmc passes of this step, averaged over the "
                                   "symbol's launches; 2 x FETCH_SIZE + WRITE_SIZE = bytes that crossed L2 <-> fabric)")
        return e

    mf = [r for r in rows if r["bound"] == "mfma"]
    hb = [r for r in rows if r["bound"] == "hbm"]
    out = {"roofline": entry(mf[0]), "roofline_other": [entry(r) for r in mf[1:6]], "roofline_hbm": [entry(r) for r in hb]}
    out["roofline"]["note"] = ("per-launch fractions are against the WHOLE chip's peak: since round 4 the 192 / 384-channel branch "
                               "convolutions launch 96 workgroups on 256 CUs by choice (less CU-time per launch, the other branches' "
                               "kernels run beside them: step -1.0 ms, profiles/r04_ab_conv_min_wgs.json), which lowers their "
                               "per-launch fraction (0.33 -> 0.22 on 12x192x32x64) while the step gets faster; `roofline_step` is the "
                               "whole step's matrix work over the timed step")
    # the whole timed step: algorithmic FLOP of every matrix-pipe launch of one step / the measured step time
    out["_step_flops"] = sum(r["flops"] for r in mf)
    if args.kernel_table:
        slim = [{k: v for k, v in r.items() if k != "shapes"} | {"shapes": {k: v[:2] for k, v in r["shapes"].items()}} for r in rows]
        with open(args.kernel_table, "w") as f:
            json.dump({"workload": workload_name(args, "step"), "timed_kernel_ms": total_ms, "rows": slim}, f, indent=1)
    return out


def roofline_gemm_kernel(args, dev, iters=10):
    """configs 4 / 5 (UPerNet + Swin): the kernel family with the largest share of the step is dcl_gemm_f16x3 behind the
    token-major Linears; `roofline` reports it on the stage-3 Mlp fc1 forward of the configured backbone (the heaviest
    Linear: tokens x C -> 4 C), timed with HIP events on the launch stream; algorithmic FLOP = 2 M N K, peak 2500 / 3."""
    from mscs_amd.models import ops
    from mscs_amd.models.amax import amax_of
    side = 640 if args.config == 5 else 512
    c = (192 if args.config == 5 else 96) * 4                   # stage-3 width
    m = args.batch * (side // 16) ** 2
    x = torch.randn(m, c, device=dev)
    w = torch.randn(4 * c, c, device=dev) * 0.05
    b = torch.zeros(4 * c, device=dev)
    amax_of(x), amax_of(w)
    ops.linear_f16x3(x, w, b, tag_out=False)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        ops.linear_f16x3(x, w, b, tag_out=False)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    flops = 2.0 * m * c * 4 * c
    achieved = flops / (ms * 1e-3) / 1e12
    # FETCH_SIZE / WRITE_SIZE per launch (KiB) of exactly these two shapes: profiles/r04_gemm_pmc.csv (tools/pmc_gemm.sh, separate
    # --pmc passes); 2 x FETCH + WRITE = bytes that crossed L2 <-> fabric
    pmc = {(16384, 384): (30987.6, 98340.6), (25600, 768): (255298.3, 307241.5)}.get((m, c))
    traffic = (2 * pmc[0] + pmc[1]) * 1024 if pmc else None
    out = {"traffic_source": "constant from profiles/r04_gemm_pmc.csv (separate rocprofv3 --pmc passes of this launch)"} if pmc else {}
    return {**out, "bound": "mfma", "kernel": f"k_gemm (dcl_gemm_f16x3): Swin stage-3 Mlp.fc1 forward, [{m} x {c}] . [{4 * c} x {c}]^T + bias",
            "achieved": round(achieved, 2), "peak": round(MFMA_F16X3_BWD_PEAK_TFLOPS, 1), "unit": "TFLOP/s",
            "frac": round(achieved / MFMA_F16X3_BWD_PEAK_TFLOPS, 4),
            "peak_note": "2 M N K algorithmic FLOP issued as 3 f16 MFMA passes (split-f16, fp32-equivalent): 2.5 PFLOP/s / 3",
            "traffic": traffic, "algorithmic_bytes": 4 * (m * c + 4 * c * c + m * 4 * c), "launch_ms": round(ms, 4)}


def roofline_bwd_kernel(mod, iters=10):
    """Average launch duration of the dominant kernel (InfoNCE backward sweep, intra-scale term 0),
    HIP events on the launch stream; algorithmic FLOPs = 4 * N1 * N2 * C (S = A B^T recompute + H B)."""
    from mscs_amd import _lib
    L = _lib.lib()
    st = mod.last_state
    t = st.terms[0]
    A = st.scales[t.a]
    N = A.plan.N
    Npad = A.bank.shape[0]
    dev = A.bank.device
    stat = torch.empty((Npad + 1, 4), device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = _lib.ptr
    _lib.check(L.dcl_infonce_prep_stats(p(t.Z), p(t.W), p(t.rng_lo), p(t.rng_hi), None, N, A.plan.V, 1, 1.0,
                                        1.0 / t.tau, None, p(stat), stream), "prep")
    ns = int(L.dcl_suggest_nsplit(N, N))
    G = int(L.dcl_infonce_bwd_streamk_workgroups(N, N)) if A.bank_h is not None else 0
    if G > 0:        # what the step runs in f16x3 mode: the stream-K partition (finished tiles, no slabs)
        dout = torch.empty((int(L.dcl_infonce_bwd_streamk_slabs(N, N)), Npad, 256), device=dev)
        ws = torch.empty((G, 128, 256), device=dev)
        flags = torch.zeros(G + 1, dtype=torch.int32, device=dev)

        def launch():
            _lib.check(L.dcl_infonce_bwd_streamk(p(A.bank), N, A.plan.V, p(A.bank), N, p(t.rng_lo), p(t.rng_hi),
                                                 1.0 / t.tau, 1, 1, 1, p(stat), p(stat), p(dout), p(ws), p(flags),
                                                 p(A.bank_h), p(A.bank_h), stream), "bwd_streamk")
    else:
        dpart = torch.empty((ns, Npad, 256), device=dev)

        def launch():
            _lib.check(L.dcl_infonce_bwd(p(A.bank), N, A.plan.V, p(A.bank), N, p(t.rng_lo), p(t.rng_hi),
                                         1.0 / t.tau, 1, 1, 1, p(stat), p(stat), ns, p(dpart), p(A.bank_h), p(A.bank_h), stream), "bwd")
    launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        launch()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    flops = 4.0 * N * N * 256
    achieved = flops / (ms * 1e-3) / 1e12
    mode = mod.DCV2_scale0.mfma_mode
    peak = MFMA_F16X3_BWD_PEAK_TFLOPS if mode == "f16x3" else MFMA_F32_PEAK_TFLOPS
    # HBM traffic per launch of this kernel at N = 9804 from the committed PMC passes (profiles/README.md):
    # (2 * FETCH_SIZE + WRITE_SIZE) KiB, FETCH doubled per the gfx950 correction in MI355X_MICROARCH.md;
    # only valid for the benchmark shape, else null
    pmc = {"f32": (102168.7, 128128.0), "f16x3": PMC_F16X3}.get(mode)       # f32 pair: round-1 f32 passes
    traffic = (2 * pmc[0] + pmc[1]) * 1024 if (pmc and N == 9804 and ns == 13 and G == 0) else None
    if G > 0 and N == 9804 and PMC_F16X3_SK:
        traffic = (2 * PMC_F16X3_SK[0] + PMC_F16X3_SK[1]) * 1024
    return {"bound": "mfma", "kernel": (f"k_sweep<MODE_BWD, stream-K> (dcl_infonce_bwd_streamk, {G} persistent workgroups)"
                                        if G > 0 else "k_sweep<MODE_BWD> (dcl_infonce_bwd)") + f", both products in {mode}",
            "achieved": round(achieved, 2), "peak": round(peak, 1), "unit": "TFLOP/s",
            "frac": round(achieved / peak, 4),
            "peak_note": ("f32 MFMA 157.3 TFLOP/s" if mode == "f32" else
                          "4NMC algorithmic FLOP issued as 3 f16 MFMA passes (split-f16, fp32-equivalent): "
                          "2.5 PFLOP/s / 3 = 833.3 TFLOP/s"),
            "traffic": traffic,
            "traffic_source": "constant from " + (PMC_SOURCE_SK if G > 0 else PMC_SOURCE) +
                              " (separate rocprofv3 --pmc run, not read live; 2 x FETCH_SIZE + WRITE_SIZE = bytes that "
                              "crossed L2 <-> fabric, Infinity-Cache hits included)",
            "algorithmic_bytes": 3 * N * 256 * 4, "launch_ms": round(ms, 4), "N1": N, "N2": N, "C": 256,
            "nsplit": ns if G == 0 else None, "streamk_workgroups": G}


PMC_HEAD_WGRAD = (3514955.5 + 19856.5, 26330.0 + 3645.0)   # k_wgrad3x3d<3,1,true> + its slab reduction, 12 x (144 -> 720) x 128 x 256
PMC_HEAD_FWD = (516063.4, 1228800.0)                        # k_conv3x3_il<3,4> on the same layer (profiles/r03_head_wgrad_pmc.csv)
PMC_F16X3 = (104540.5, 128128.0)      # KiB per launch (FETCH_SIZE, WRITE_SIZE), profiles/r02_loss_pmc_*.csv
PMC_F16X3_SK = (60279.9, 71687.9)     # stream-K kernel with 4 column slices, KiB per launch: profiles/r05_loss_pmc_fetch.csv / _write.csv (60285.2 there)
                                      # (one slice, round 3's partition, same run: 281075.0 / 42504.0 -- r04_loss_pmc_*_1slice.csv)
PMC_SOURCE = "profiles/r02_loss_pmc_fetch.csv, r02_loss_pmc_write.csv"
PMC_SOURCE_SK = "profiles/r05_loss_pmc_fetch.csv, r05_loss_pmc_write.csv"


def host_threads():
    """Host threads of the CPU baseline: every core up to 64, or the OMP_NUM_THREADS budget where one is set."""
    budget = int(os.environ.get("OMP_NUM_THREADS") or 0) or 64
    return max(1, min(os.cpu_count() or 1, 64, budget))


def cpu_baseline_loss(args):
    """oracle/eager_torch.py (the eager-structure restatement: per-(image, class) Python loop, host randperm, N x N
    matrices, autograd index-backward) on the host cores: ONE evaluation of the WHOLE loss of the workload -- every
    scale's sampling + intra-scale term and every cross-scale term, forward and backward -- after a warm-up on one small
    term.  Nothing is multiplied: the seconds reported are the seconds measured.  Returns (seconds, threads, description)."""
    from oracle import eager_torch
    threads = host_threads()
    torch.set_num_threads(threads)
    gen = torch.Generator().manual_seed(0)
    n, H, W, S = args.batch, args.height, args.width, args.scales
    label = torch.randint(0, args.classes, (n, H, W), generator=gen)
    feats = [torch.randn(n, 256, H // (4 << s), W // (4 << s), generator=gen).requires_grad_(True) for s in range(S)]
    w = [1.0, 0.7, 0.4, 0.1][:S]
    torch.manual_seed(0)
    warm = feats[-1].detach().clone().requires_grad_(True)          # warm-up: thread pool, allocator (one coarse term)
    bank, classes = eager_torch.sample_bank(label, warm, args.classes, 5, 2500, 2000)
    eager_torch.intra_loss(bank, classes, 0.1).backward()
    t0 = time.perf_counter()
    total, ms, cs = eager_torch.dcv2_ms(label, feats, args.classes, 0.1, w, cross=not args.no_cross)
    total.backward()
    dt = time.perf_counter() - t0
    return dt, threads, (f"loss: ONE evaluation of the whole DenseContrastiveLossV2_ms ({S} scales + {len(cs)} cross-scale "
                         f"term(s), batch {n}, {H}x{W}, C=256) fwd+bwd, eager torch fp32 on {threads} host threads after a "
                         f"warm-up term = {dt:.2f} s measured (not extrapolated)")


def cpu_baseline_model(args, micro=4):
    """HRNet-W48 + projector + CE forward / backward / SGD over ALL `batch` images of the benchmark size on the host cores
    (stock PyTorch CPU, fp32), in micro-batches of `micro` images with gradient accumulation (host memory: a batch-12
    activation set of this model is ~50 GB) -- every image is computed, nothing is multiplied -- after a one-image warm-up.
    Returns (seconds for the whole batch, description)."""
    import mscs_amd  # noqa: F401
    from mscs_amd.models import HRNet
    threads = host_threads()
    torch.set_num_threads(threads)
    graph = {"backbone": "hrnet48", "pretrained": False, "dataset": "CITYSCAPES", "align_corners": True,
             "ms_projector": {"mlp": [[1, -1, 1]], "scales": args.scales, "d": 256, "use_bn": True}}
    model = HRNet(graph, 1)
    opt = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=5e-4)
    gen = torch.Generator().manual_seed(0)
    img = torch.randn(args.batch, 3, args.height, args.width, generator=gen)
    lbl = torch.randint(0, 20, (args.batch, args.height, args.width), generator=gen)
    ce = torch.nn.CrossEntropyLoss(ignore_index=19)

    def fwd_bwd(lo, hi):
        out, proj = model(img[lo:hi])
        loss = ce(out, lbl[lo:hi]) + sum(p.mean() for p in proj) * 0.0
        loss.backward()

    fwd_bwd(0, 1)                                            # warm-up (thread pool, oneDNN primitives)
    opt.zero_grad()
    t0 = time.perf_counter()
    for lo in range(0, args.batch, micro):
        fwd_bwd(lo, min(lo + micro, args.batch))
    opt.step()
    dt = time.perf_counter() - t0
    return dt, (f"model: HRNet-W48 + projector + CE fwd+bwd over all {args.batch} images {args.height}x{args.width} "
                f"(micro-batches of {micro}, gradient accumulation) + one SGD step, torch CPU fp32 on {threads} threads after "
                f"a one-image warm-up = {dt:.2f} s measured (not extrapolated)")


def workload_name(args, workload):
    cross = "" if args.no_cross else " + cross-scale"
    if workload == "loss":
        return (f"DenseContrastiveLossV2_ms fwd+bwd, {args.scales} scales{cross}, n={args.batch} "
                f"{args.height}x{args.width} {args.labels} labels K={args.classes}, C=256, per GPU")
    if args.config in (4, 5):
        which = "configs[3] on one GPU (SURVEY App. C 4'): UPerNet + Swin-T" if args.config == 4 else \
            "configs[4] on one GPU: UPerNet + Swin-L"
        return (f"BASELINE {which} + LossWrapper(TwoScaleLoss + "
                f"0.1*DenseContrastiveLossV2_ms, {args.scales} scales{cross}, fpn projector) train step (fwd+bwd+AdamW), "
                f"synthetic ADE20K {args.height}x{args.width}, batch {args.batch} per GPU, {args.labels} labels")
    return (f"HRNet-W48 + LossWrapper(CE + 0.1*DenseContrastiveLossV2_ms, {args.scales} scales{cross}) train step "
            f"(fwd+bwd+SGD), synthetic Cityscapes {args.height}x{args.width}, batch {args.batch} per GPU, {args.labels} labels")


def opt_out_keys(args):
    """The graph block of the timed step holds the REFERENCE's keys only: this package's managers turn the fused consumers
    (graph.lazy_logits, graph.lazy_projector) on by themselves when the loss is their own LossWrapper (BaseManager.load_model).
    --materialize-logits / --materialize-projector / --plain-config write the explicit `false` that hands out the reference's
    tensors instead."""
    keys = {}
    if args.materialize_logits or args.plain_config:
        keys["lazy_logits"] = False
    if getattr(args, "materialize_projector", False) or args.plain_config:
        keys["lazy_projector"] = False
    return keys


def fused_opt_key(args):
    if args.plain_config or os.environ.get("DCL_FUSED_OPT", "1") == "0":
        return {"fused_optimizer": False}       # torch's default (foreach) parameter update
    return {}


def step_config_upernet(args, world):
    """configs/ADE20K/upnswin_contrastive_ADE20K.json of the reference (graph / loss / train blocks as shipped), on the
    synthetic dataset."""
    S = args.scales
    return {
        "name": "bench4", "mode": "training", "manager": "OCRNet", "cuda": True, "seed": 0,
        "parallel": world > 1, "batch_is_global": False,
        "graph": {"model": "UPerNet", "backbone": "swinL" if args.config == 5 else "swinT", "sync_bn": True, "out_stride": 32, "pretrained": False,
                  "align_corners": False, "aux_head": {"in_index": 3, "dropout_rate": 0.1}, "dropout_rate": 0.1,
                  **opt_out_keys(args),
                  "ms_projector": {"mlp": [[1, -1, 1]], "scales": S, "d": 256, "use_bn": True, "position": "fpn"}},
        "data": {"dataset": "ADE20K", "experiment": 1, "batch_size": args.batch, "num_workers": 0,
                 "synthetic": True, "synthetic_length": args.batch * 2,
                 "transform_values": {"crop_shape": [args.height, args.width]}},
        "loss": dict(loss_config(S, not args.no_cross, "ADE20K"), name="LossWrapper",
                     interm={"name": "CrossEntropyLoss", "args": [], "weight": 0.4},
                     final={"name": "CrossEntropyLoss", "args": [], "weight": 1.0},
                     losses={"TwoScaleLoss": 1.0, "DenseContrastiveLossV2_ms": 0.1}),
        "train": {**fused_opt_key(args),
                  "lr_batchwise": True, "learning_rate": 0.00006, "lr_fct": "linear-warmup-polynomial",
                  "lr_params": {"power": 1.0, "warmup_iters": 1500, "warmup_rate": 1e-6, "min_lr": 0.0},
                  "optim": "AdamW", "epochs": 127, "momentum": 0.9, "betas": [0.9, 0.999], "weight_decay": 0.01,
                  "opt_keys": {"absolute_pos_embed": {"wd_mult": 0.0}, "norm": {"wd_mult": 0.0},
                               "relative_position_bias_table": {"wd_mult": 0.0}}},
    }


def step_config(args, world):
    if getattr(args, "config", 2) in (4, 5):
        return step_config_upernet(args, world)
    S = args.scales
    return {
        "name": "bench", "mode": "training", "manager": "HRNet", "cuda": True, "seed": 0,
        "parallel": world > 1, "batch_is_global": False, "channels_last": args.channels_last,
        "graph": {"model": "HRNet", "backbone": "hrnet48", "sync_bn": True, "out_stride": 4, "pretrained": False,
                  "align_corners": True, "branch_conv": args.branch_conv, **opt_out_keys(args),
                  "conv1x1": getattr(args, "conv1x1", "f16x3"),
                  "ms_projector": {"mlp": [[1, -1, 1]], "scales": S, "d": 256, "use_bn": True, "before_context": True}},
        "data": {"dataset": "CITYSCAPES", "experiment": 1, "batch_size": args.batch, "num_workers": 0,
                 "synthetic": True, "synthetic_length": args.batch * 2,
                 "transform_values": {"crop_shape": [args.height, args.width]}},
        "loss": dict(loss_config(S, not args.no_cross), name="LossWrapper",
                     losses={"CrossEntropyLoss": 1, "DenseContrastiveLossV2_ms": 0.1}),
        "train": {**fused_opt_key(args),
                  "learning_rate": 0.01, "lr_fct": "polynomial", "optim": "SGD", "lr_batchwise": True,
                  "epochs": 484, "momentum": 0.9, "weight_decay": 0.0005},
    }


def time_train_step(args, dev, rank, world):
    """K training steps of HRNetManager on one resident synthetic batch per rank."""
    import mscs_amd  # noqa: F401
    from mscs_amd.managers import HRNetManager, OCRNetManager
    from mscs_amd.utils import set_verbosity
    set_verbosity(40)
    torch.backends.cudnn.benchmark = bool(args.miopen_benchmark)
    mgr = (OCRNetManager if args.config in (4, 5) else HRNetManager)(step_config(args, world), autostart=False)
    mgr.setup()
    mgr.model.train()
    gen = torch.Generator().manual_seed(1000 * rank)
    img = torch.randn(args.batch, 3, args.height, args.width, generator=gen).to(dev)
    lbl = synth_labels(args, args.batch, args.height, args.width, gen).to(dev)  # int64
    if args.channels_last:
        img = img.contiguous(memory_format=torch.channels_last)
    amp = torch.autocast("cuda", dtype=torch.bfloat16) if args.amp else contextlib.nullcontext()
    torch.cuda.synchronize()
    ready = torch.cuda.Event()          # inputs are resident before the timed region: "label complete" has fired
    ready.record()

    def step(i=0):
        # exactly BaseManager.train_one_epoch's loop body on a resident batch: forward, loss, backward, SGD, LR
        # schedule, then the per-step metrics tail of the reference (HRNet_Manager.py:117-121)
        mgr.optimiser.zero_grad(set_to_none=True)
        with amp:
            ret = mgr.forward_step(img, lbl, label_ready=ready)
        ret["loss"].backward()
        mgr.optimiser.step()
        mgr.scheduler.step()
        if not args.no_metrics:
            mgr.step_metrics(1, ret, lbl, 0.0)
        return ret

    for _ in range(args.warmup):
        step()
    sync(world)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        ret = step()
    sync(world)
    dt = time.perf_counter() - t0
    mgr.flush_logging()
    # a timing of a run whose numbers went bad is not a measurement (a chip multiplying NaNs even clocks higher):
    # the last loss and every parameter must be finite after the timed steps
    bad = [n for n, p in mgr.model.named_parameters() if not torch.isfinite(p).all()]
    if bad or not torch.isfinite(ret["loss"]).item():
        raise RuntimeError(f"benchmark step diverged: loss {float(ret['loss'])}, non-finite parameters {bad[:5]}")
    mod = mgr.loss.loss_classes["DenseContrastiveLossV2_ms"]
    extra = {}
    if args.full:
        extra["contrastive_loss_fwd_bwd_ms"] = round(loss_only_ms(mod, dev, args), 3)
    extra.update({"metrics_in_step": not args.no_metrics,
             # one resident batch, its "label complete" event fired before the timed region: the label stage of step i + 1 overlaps
             # step i's tail, which a dataloader-fed run cannot do for the first ~1.5 ms of a step
             "timed_batch": "resident; label_ready pre-fired",
             # what the manager resolved (the timed config itself holds reference keys only unless a --materialize-* /
             # --plain-config flag wrote an explicit `false`): logits kept at 1/4 resolution for the fused up-sampling +
             # cross-entropy / arg-max kernels
             "lazy_logits": bool(mgr.config["graph"].get("lazy_logits", False)),
             # the projection heads' last 1x1 convolution evaluated on the sampled pixels only (models/Projector.LazyProjection)
             "lazy_projector": bool(mgr.config["graph"].get("lazy_projector", False)),
             "fused_optimizer": bool(getattr(mgr.optimiser, "defaults", {}).get("fused", False)),
             "config_keys_beyond_reference": sorted(set(opt_out_keys(args)) | set(fused_opt_key(args))),
             "model_dtype": "bf16-autocast" if args.amp else "f32",
             "memory_format": "channels_last" if args.channels_last else "contiguous",
             "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)})
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, step_outputs(mgr, ret, args))
    if args.full and not getattr(args, "no_kernel_table", False) and world == 1:
        # ONE more step, serialised: every launch on the main stream (no branch streams, no side stream in the head's backward),
        # so that the two HIP events around a launch bracket that kernel and nothing else -- with one stream per branch an event
        # pair also counts the time the launch waits for CUs held by the other streams' kernels (measured: 165 us per weight-
        # gradient launch against 87 us in rocprofv3's trace of the same step).  Same kernels, shapes, tiles and data as the timed
        # steps; the per-kernel durations of the timed (multi-stream) schedule are in profiles/r04_step_kernels.csv.
        from mscs_amd.utils.kernel_timer import KernelTimer
        import importlib
        _hr = importlib.import_module("mscs_amd.models.HRNet")     # (the module: the package re-exports the class under this name)
        from mscs_amd.debug import cfg as _dbg
        from mscs_amd.models import ops as _ops
        keep = (_hr._BRANCH_STREAMS, _dbg.head_overlap, _ops._HeadSplit.overlap)
        _hr._BRANCH_STREAMS, _dbg.head_overlap, _ops._HeadSplit.overlap = False, 0, 0
        try:
            step()                                   # (allocator / stream state settles)
            torch.cuda.synchronize()
            with KernelTimer() as kt:
                step()
                torch.cuda.synchronize()
        finally:
            _hr._BRANCH_STREAMS, _dbg.head_overlap, _ops._HeadSplit.overlap = keep
        extra["_kernel_rows"] = kt.rows()
    del mgr
    return dt, mod, extra


def loss_only_ms(mod, dev, args, iters=5):
    """Contrastive-loss fwd+bwd alone on projector-shaped synthetic features (same labels/config as the
    step), wall time per evaluation including its host-side planning."""
    label, feats = synth_loss_inputs(args, dev, 0)
    def run():
        for f in feats:
            f.grad = None
        mod(label, feats).backward()
    run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def self_launch(args):
    """``python bench.py --gpus N`` (N > 1) started WITHOUT a launcher (no WORLD_SIZE in the environment): start the N
    ranks ourselves -- ``python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1`` on
    this very command line, as a CHILD process and before anything in this process has touched the GPU -- forward
    rank 0's single JSON line and exit with the child's code.  (Under the driver's own torch.distributed.run launch
    WORLD_SIZE is set and this is skipped.)"""
    import socket
    import subprocess
    have = torch.cuda.device_count()            # counting devices does not initialise the GPU
    rehearsal = os.environ.get("DCL_BENCH_REHEARSAL") == "1"
    if have < args.gpus and not rehearsal:
        raise SystemExit(f"bench.py --gpus {args.gpus}: only {have} GPU(s) visible on this node "
                         f"(DCL_BENCH_REHEARSAL=1 rehearses the {args.gpus}-rank launch on one GPU over gloo; "
                         f"its number is not a measurement)")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return subprocess.call(cmd, env=env)

LINE_LIMIT = 4096       # the driver keeps a ~9 KB stdout tail (a 23.7 KB line was recorded as "parsed": null)
_ROOF_KEYS = ("bound", "kernel", "achieved", "peak", "unit", "frac", "launches", "launch_ms", "step_ms", "algorithmic_flops",
              "algorithmic_bytes", "traffic")
_TOP_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
             "dtype", "data", "config", "contrastive_loss_fwd_bwd_ms", "roofline", "roofline_step", "roofline_sweep", "cpu_baseline",
             "eager_gpu_step_ms", "speedup_vs_eager_gpu_step", "eager_gpu_step_ms_miopen_find", "plain_config_ms_per_step",
             "metrics_in_step", "lazy_logits", "lazy_projector", "fused_optimizer", "config_keys_beyond_reference", "peak_mem_gb",
             "timed_batch", "detail")


def _short_kernel(name):
    """'k_conv3x3_il<3,4> (dcl_conv3x3_f16x3): all 242 launches ...' -> 'k_conv3x3_il<3,4> (dcl_conv3x3_f16x3)'"""
    cut = name.find("):")
    name = name[:cut + 1] if cut > 0 else name
    return name[:96]


def _slim_roofline(r):
    if not r:
        return r
    e = {k: r[k] for k in _ROOF_KEYS if k in r}
    e["kernel"] = _short_kernel(str(e.get("kernel", "")))
    for k in ("algorithmic_flops", "algorithmic_bytes", "traffic"):
        if isinstance(e.get(k), float):
            e[k] = float(f"{e[k]:.5g}")
    return e


def compact_line(full):
    """The ONE stdout line the driver parses: BASELINE.json's metric, one `roofline`, `roofline_step`, the similarity sweep's
    roofline (the kernel north_star names), a `cpu_baseline` and the comparator ratios -- no per-shape tables, no prose.
    Everything else (`roofline_other`, `roofline_hbm`, shapes, notes) is the detail record (stderr / --detail-file).
    Guaranteed <= LINE_LIMIT bytes: optional keys are dropped, last first, until it fits."""
    line = {k: full[k] for k in _TOP_KEYS if k in full}
    if "config" in line:
        line["config"] = {"workload": str(full["config"].get("workload", ""))[:300]}
    for k in ("roofline", "roofline_step"):
        if k in line:
            line[k] = _slim_roofline(line[k])
    sweep = [r for r in full.get("roofline_other", []) if "k_sweep" in str(r.get("kernel", ""))]
    if sweep and "roofline_sweep" not in line and "k_sweep" not in str(full.get("roofline", {}).get("kernel", "")):
        line["roofline_sweep"] = _slim_roofline(sweep[0])
    cb = full.get("cpu_baseline")
    if cb:
        line["cpu_baseline"] = {k: cb[k] for k in ("value", "unit", "cores", "kind", "sample_count", "sample_seconds", "model_seconds",
                                                   "loss_seconds") if k in cb}
        line["cpu_baseline"]["sample"] = str(cb.get("sample_short") or cb.get("sample", ""))[:200]
    drop = ["peak_mem_gb", "config_keys_beyond_reference", "fused_optimizer", "lazy_projector", "lazy_logits", "metrics_in_step",
            "eager_gpu_step_ms_miopen_find", "detail", "roofline_sweep", "timed_batch"]
    text = json.dumps(line)
    while len(text) >= LINE_LIMIT and drop:
        line.pop(drop.pop(0), None)
        text = json.dumps(line)
    if len(text) >= LINE_LIMIT:
        raise RuntimeError(f"bench line is {len(text)} bytes (limit {LINE_LIMIT}): {sorted(line)}")
    return text


def emit(full, args):
    """detail record -> stderr (+ --detail-file), compact line -> stdout, LAST."""
    detail = json.dumps(full)
    if getattr(args, "detail_file", None):
        with open(args.detail_file, "w") as f:
            f.write(detail + "\n")
        full = dict(full, detail=args.detail_file)
    print("bench-detail: " + detail, file=sys.stderr, flush=True)
    print(compact_line(full), flush=True)


def main():
    args = parse()
    global MFMA_MODE
    MFMA_MODE = args.mfma
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py --gpus {args.gpus} launched with WORLD_SIZE={world}: the two must agree")
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    rehearsal = world > 1 and os.environ.get("DCL_BENCH_REHEARSAL") == "1"
    if rehearsal:
        # dress rehearsal of the N-rank launch on a box with ONE GPU: every rank on cuda:0, gloo instead of RCCL (which
        # refuses two ranks on one device).  Exercises the launch contract, DDP, SyncBN and the max-over-ranks timing;
        # the number it prints is not a measurement.
        local = 0
        os.environ["LOCAL_RANK"] = "0"
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local)
        # one host core per rank is what the launch loop needs; leave the rest to the other ranks
        torch.set_num_threads(max(1, (os.cpu_count() or world) // world))
        dist.init_process_group("gloo" if rehearsal else "nccl", rank=rank, world_size=world)
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    workload = args.workload or "step"

    extra = {}
    if workload == "loss":
        dt, mod = time_loss_only(args, dev, rank, world)
        unit_per_step = 1.0
        metric, unit = "contrastive_loss_fwd_bwd_per_sec", "loss evals/s"
    else:
        dt, mod, extra = time_train_step(args, dev, rank, world)
        unit_per_step = float(args.batch)
        metric, unit = "train_images_per_sec", "images/s"

    tmax = torch.tensor([dt], device=dev)
    if world > 1:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    dt = float(tmax.item())
    ms_per_step = dt / args.steps * 1e3
    value = world * unit_per_step * args.steps / dt

    out = None
    if rank == 0:
        n_terms = len(mod.last_state.terms)
        out = {
            "metric": metric, "value": round(value, 3), "unit": unit, "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32 (f16x3-emulated)" if (MFMA_MODE or "f16x3") == "f16x3" else "f32",
            "data": "synthetic",
            "config": {"workload": workload_name(args, workload),
                       "terms": [[t.a, t.b, st_n(mod, t.a), st_n(mod, t.b)] for t in mod.last_state.terms]},
        }
        out.update(extra)
        if workload == "loss":
            out["contrastive_loss_fwd_bwd_ms"] = round(ms_per_step, 3)
        if args.full:
            full_measurements(out, extra, args, dev, mod, workload, world, ms_per_step)
        out.pop("_kernel_rows", None)
        emit(out, args)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def full_measurements(out, extra, args, dev, mod, workload, world, ms_per_step):
    """--full: what the benchmark measures beyond the headline (each part runs work of its own after the timed steps):
    roofline / per-kernel figures, the host CPU baseline, the plain-config step and the eager comparators (rank 0)."""
    unit = out["unit"]
    if workload == "loss":
        out["roofline"] = roofline_bwd_kernel(mod)
    elif args.config != 2:
        rows = extra.pop("_kernel_rows", None)
        out.pop("_kernel_rows", None)
        out["roofline"] = roofline_gemm_kernel(args, dev)
        out["roofline_other"] = [roofline_bwd_kernel(mod)]
        if rows:
            tab = roofline_from_rows(rows, args)
            tab.pop("_step_flops", None)
            out["roofline_other"] += [tab["roofline"]] + tab["roofline_other"][:4]
            out["roofline_hbm"] = tab["roofline_hbm"]
    else:
        rows = extra.pop("_kernel_rows", None)
        head_main, head_others = roofline_conv_kernels(args, dev)
        if rows:
            out.update(roofline_from_rows(rows, args))
            out["roofline_other"] += [head_main] + head_others[:1] + [roofline_bwd_kernel(mod)]
            fl = out.pop("_step_flops")
            ach = fl / (ms_per_step * 1e-3) / 1e12
            out["roofline_step"] = {"bound": "mfma", "kernel": "all matrix-pipe launches of one training step (direct convolutions, "
                                    "weight gradients, split-f16 GEMMs, similarity sweeps) over the TIMED multi-stream step",
                                    "algorithmic_flops": fl, "achieved": round(ach, 2), "peak": round(MFMA_F16_PEAK_TFLOPS / 3.0, 1),
                                    "unit": "TFLOP/s", "frac": round(ach / (MFMA_F16_PEAK_TFLOPS / 3.0), 4),
                                    "note": "the step also holds ~30 ms of HBM-bound kernels (roofline_hbm) on the same streams"}
        else:
            out["roofline"] = head_main
            out["roofline_other"] = head_others + [roofline_bwd_kernel(mod)]
    out.pop("_kernel_rows", None)
    if not args.no_cpu_baseline and world == 1 and args.config == 2:    # host baseline: single-GPU headline run only
        lsec, cores, lsample = cpu_baseline_loss(args)
        if workload == "loss":
            out["cpu_baseline"] = {"value": round(1.0 / lsec, 5), "unit": unit, "cores": cores,
                                   "kind": "port", "sample": lsample, "sample_seconds": round(lsec, 2),
                                   "sample_count": 1,      # ONE evaluation (tens of seconds), not the median of three
                                   "sample_short": f"one whole DCV2_ms evaluation fwd+bwd ({args.scales} scales + cross-scale, batch "
                                                   f"{args.batch}, {args.height}x{args.width}), eager torch fp32, measured once"}
        else:
            msec, msample = cpu_baseline_model(args)
            out["cpu_baseline"] = {"value": round(args.batch / (msec + lsec), 5), "unit": unit, "cores": cores,
                                   "kind": "port", "sample": msample + "; " + lsample,
                                   "sample_count": 1,      # ONE whole step (~70 s of host time), not the median of three: SURVEY
                                                           # section 8d's three would take the default run past its few minutes
                                   "model_seconds": round(msec, 2), "loss_seconds": round(lsec, 2),
                                   "sample_seconds": round(msec + lsec, 2),
                                   "sample_short": f"one whole step: HRNet-W48 fwd+bwd over all {args.batch} images (micro-batches "
                                                   f"of 4) + SGD + one full DCV2_ms evaluation, torch CPU fp32, measured once"}
    if workload == "step" and world == 1 and not args.no_reference_config and not args.plain_config:
        # the same step with this package's opt-in behaviour switched OFF by explicit `false` keys: full-resolution logits,
        # the projector's [n, d, h, w] maps (pixel-major strides), torch's foreach optimizer -- what a user gets who calls the
        # model classes directly / writes the keys; the timed headline config holds reference keys only
        import copy
        a2 = copy.copy(args)
        a2.plain_config, a2.no_kernel_table, a2.kernel_table, a2.dump_outputs = True, True, None, None
        torch.cuda.empty_cache()
        dt2, _, ex2 = time_train_step(a2, dev, 0, world)
        out["plain_config_ms_per_step"] = round(dt2 / args.steps * 1e3, 3)
        out["plain_config_keys"] = ex2["config_keys_beyond_reference"]
        torch.cuda.empty_cache()
    if args.eager_baseline:
        out["eager_gpu_loss_ms"] = round(eager_gpu_loss_ms(args, dev), 2)
    if workload == "step" and world == 1 and not args.no_eager_step and args.config == 2:
        torch.cuda.empty_cache()
        eager_ms = eager_gpu_step_ms(args, dev)
        out["eager_gpu_step_ms"] = round(eager_ms, 1)
        out["speedup_vs_eager_gpu_step"] = round(eager_ms / ms_per_step, 2)
        out["eager_gpu_step_note"] = ("same architecture on stock PyTorch-ROCm kernels (MIOpen / ATen, one stream) + "
                                      "eager-structure contrastive loss (oracle/eager_torch.py) + SGD, same GPU, "
                                      "median of 3 after 1 warm-up; BASELINE.json target: >= 5x; "
                                      "torch.backends.cudnn.benchmark off (MIOpen's immediate-mode solvers) -- "
                                      "--eager-miopen-benchmark adds the reference's benchmark=True setting; the "
                                      "comparator has no per-step metrics tail, the timed step does")
        if args.eager_miopen_benchmark:
            t0 = time.perf_counter()
            tuned_ms = eager_gpu_step_ms(args, dev, miopen_benchmark=True)
            out["eager_gpu_step_ms_miopen_find"] = round(tuned_ms, 1)
            out["speedup_vs_eager_gpu_step_miopen_find"] = round(tuned_ms / ms_per_step, 2)
            out["eager_miopen_find_total_s"] = round(time.perf_counter() - t0, 1)


def eager_gpu_step_ms(args, dev, iters=3, miopen_benchmark=False):
    """The "reference PyTorch-eager GPU step" of BASELINE.json's >= 5x target (SURVEY.md section 8 row d), measured
    on THIS MI355X in the same run: the same HRNet-W48 + projector architecture on stock PyTorch-ROCm kernels only
    (MIOpen convolutions and batch norm, ATen interpolate, one stream; mscs_amd.models.ops.library_kernels_only),
    torch's CrossEntropyLoss, and the eager-structure restatement of the contrastive loss (oracle/eager_torch.py:
    the reference's per-(image, class) Python loop with .item() indexing, nonzero, host randperm, N x N matrices
    and autograd index-backward), SGD step.  Same batch, same labels; median of ``iters`` after one warm-up step
    (which also absorbs MIOpen's kernel selection)."""
    import mscs_amd  # noqa: F401
    from mscs_amd.models import HRNet
    from mscs_amd.models.ops import library_kernels_only
    from oracle import eager_torch
    S = args.scales
    graph = {"backbone": "hrnet48", "pretrained": False, "dataset": "CITYSCAPES", "align_corners": True,
             "branch_conv": "library", "head_conv": "library", "fused_bn": False, "gemm_conv1x1": False, "conv1x1": "library",
             "ms_projector": {"mlp": [[1, -1, 1]], "scales": S, "d": 256, "use_bn": True}}
    torch.backends.cudnn.benchmark = bool(miopen_benchmark)
    model = HRNet(graph, 1).to(dev).train()
    opt = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=5e-4)
    gen = torch.Generator().manual_seed(0)
    img = torch.randn(args.batch, 3, args.height, args.width, generator=gen).to(dev)
    lbl = synth_labels(args, args.batch, args.height, args.width, gen).to(dev)
    ce = torch.nn.CrossEntropyLoss(ignore_index=19)
    w = [1.0, 0.7, 0.4, 0.1][:S]
    times = []
    with library_kernels_only():
        for it in range(iters + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            opt.zero_grad(set_to_none=True)
            out, proj = model(img)
            dc, _, _ = eager_torch.dcv2_ms(lbl, proj, 20, 0.1, w, cross=not args.no_cross)
            loss = ce(out, lbl) + 0.1 * dc
            loss.backward()
            opt.step()
            torch.cuda.synchronize()
            if it:
                times.append((time.perf_counter() - t0) * 1e3)
    if not torch.isfinite(loss).item():
        raise RuntimeError(f"eager comparator diverged: loss {float(loss)}")
    del model, opt
    torch.cuda.empty_cache()
    torch.backends.cudnn.benchmark = False
    return sorted(times)[len(times) // 2]


def st_n(mod, s):
    return mod.last_state.scales[s].plan.N


def eager_gpu_loss_ms(args, dev):
    """The eager-structure restatement of the loss (oracle/eager_torch.py) on the MI355X."""
    from oracle import eager_torch
    gen = torch.Generator().manual_seed(0)
    n, H, W = args.batch, args.height, args.width
    label = synth_labels(args, n, H, W, gen).to(dev)
    feats = [torch.randn(n, 256, H // (4 << s), W // (4 << s), generator=gen).to(dev).requires_grad_(True)
             for s in range(args.scales)]
    w = [1.0, 0.7, 0.4, 0.1][:args.scales]

    def step():
        for f in feats:
            f.grad = None
        total, _, _ = eager_torch.dcv2_ms(label, feats, 20, 0.1, w, cross=not args.no_cross)
        total.backward()
    step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / 2 * 1e3


if __name__ == "__main__":
    main()
