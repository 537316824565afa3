"""Training driver and device-side evaluation passes.  The step functions reproduce the reference's step order on one rank
(train.py:119-155 source step, :211-250 target step, :266-298 loop body, base_trainer.py:47-73 optimiser factory) with their batch exchange, the synthetic workload and the checkpoints; the evaluation passes run the network
and the count kernels: label-map inference, validation, sample weights, activation probes, class features and the epoch panels.
The host-side readers and renderers of the tables those passes return live in reports.py and are re-exported here: callers use
`driver.<name>`.  Works on the bare module or on a DistributedDataParallel wrapper (backend "nccl" == RCCL on ROCm)."""
import contextlib

import torch

from reports import (  # noqa: F401  (the public surface of this module)
    activation_report, class_gap_report, class_subset_mean, counts_from_confusion, domain_gap_report, format_activation_report,
    format_boundary, format_class_gap_report, format_confusion, format_consistency, format_domain_gap_report, format_gradient_report,
    format_segments, gradient_report, moment_gap, pseudo_label_audit, skipped_step_report, stat_mean, summarise_boundary,
    summarise_confusion, summarise_consistency, summarise_iou, summarise_reliability, summarise_segments, summarise_validation)
from visualise import FixedBatches  # noqa: F401  (`save_fixed_batch` / `has_fixed_batch`, base_trainer.py:200-218)


def _unwrap(net):
    """The module behind a DistributedDataParallel / OverlappedDataParallel wrapper (`.module`), or `net` itself."""
    return net.module if hasattr(net, "module") else net


@contextlib.contextmanager
def eval_mode(module):
    """Switches `module` to eval mode for the block and restores the mode it was in, also when the block raises."""
    was = module.training
    module.eval()
    try:
        yield module
    finally:
        module.train(was)


def rank_sum(tensor):
    """Sums `tensor` over the ranks of the process group, in place, and returns it; without a process group of more than one rank
    nothing happens.  gloo reads a device tensor with no ordering against the stream that fills it (see prep_batch), so under gloo
    the HOST copy is summed and returned; RCCL sums on the device, stream-ordered."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return tensor
    if dist.get_backend() == "gloo":
        tensor = tensor.cpu()
    dist.all_reduce(tensor)
    return tensor


def make_optimizer(net, cfg_model, fused=True, max_grad_norm=None, skip_nonfinite=False, tensor_stats=False):
    """`BaseTrainer.get_optim` (base_trainer.py:47-73) over the model's four parameter groups (train.py:93-96):
      OPT == "SGD" (the default, configs/*.yaml): SGD(momentum, nesterov=OPT_NESTEROV) -- the fused multi-tensor HIP optimiser
          (same update rule / state layout) for plain momentum or, with fused=False / nesterov, torch.optim.SGD itself;
      OPT == "Adam": torch.optim.Adam(lr, betas=(BETA1, 0.999), weight_decay) (base_trainer.py:57-61);
      any other name in torch.optim: optim(params, lr=LR) (base_trainer.py:68-69); unknown names raise NotImplementedError.
    fused="all" also returns the HIP optimisers for the other two cases of the factory: `FusedSGD(nesterov=True)` under
    OPT_NESTEROV and `FusedAdam` under OPT == "Adam" (anything else as under fused=True).
    max_grad_norm / skip_nonfinite: global L2 gradient-norm clipping and skipping of a step whose gradient norm is Inf / NaN,
    inside the fused optimisers (dasac_hip/optim.py; `optim.grad_norm` and `optim.skipped_steps` are device tensors).  Either
    one implies fused="all", so that all three cases of the factory have it; ValueError with fused=False or an OPT that has no
    fused class.
    tensor_stats: the per-tensor gradient health table of the fused optimisers (`track_tensor_stats`: `optim.tensor_stats`,
    `optim.last_skipped_stats`; read it with `gradient_report` / `skipped_step_report`), under the same rules.
    Every group carries its own lr / weight_decay (basenet.py:102-139), so the keyword defaults below only fill the gaps,
    exactly as in the reference."""
    core = _unwrap(net)
    groups = core.parameter_groups(cfg_model.LR, cfg_model.WEIGHT_DECAY)
    opt = getattr(cfg_model, "OPT", "SGD")
    if not hasattr(torch.optim, opt):
        print("Optimiser {} not supported".format(opt))
        raise NotImplementedError
    guard = {}
    if max_grad_norm is not None or skip_nonfinite or tensor_stats:
        if not fused or opt not in ("SGD", "Adam"):
            raise ValueError("max_grad_norm / skip_nonfinite / tensor_stats live in the fused optimisers: not with fused=False or "
                             "OPT == {!r}".format(opt))
        fused, guard = "all", dict(max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite)
        if tensor_stats:
            guard["track_tensor_stats"] = True
    fuse_all = isinstance(fused, str) and fused == "all"
    if opt == "Adam":
        betas = (getattr(cfg_model, "BETA1", 0.5), 0.999)
        if fuse_all:
            from dasac_hip.optim import FusedAdam
            upd = FusedAdam(groups, lr=cfg_model.LR, betas=betas, weight_decay=cfg_model.WEIGHT_DECAY, **guard)
        else:
            upd = torch.optim.Adam(groups, lr=cfg_model.LR, betas=betas, weight_decay=cfg_model.WEIGHT_DECAY)
    elif opt == "SGD":
        nesterov = getattr(cfg_model, "OPT_NESTEROV", False)
        if fused and (fuse_all or not nesterov):
            from dasac_hip.optim import FusedSGD
            upd = FusedSGD(groups, lr=cfg_model.LR, momentum=cfg_model.MOMENTUM, weight_decay=cfg_model.WEIGHT_DECAY, nesterov=nesterov,
                           **guard)
        else:
            upd = torch.optim.SGD(groups, lr=cfg_model.LR, momentum=cfg_model.MOMENTUM, nesterov=nesterov, weight_decay=cfg_model.WEIGHT_DECAY)
    else:
        upd = getattr(torch.optim, opt)(groups, lr=cfg_model.LR)
    upd.zero_grad()
    return upd


def train_epoch(net, optim, loader_source, loader_target, cfg_model, group_size, target_only=False, on_iteration=None):
    """The loop body of `Trainer.train_epoch` (train.py:266-298) -- the per-iteration POLICY around the two step functions:
    baseline mode runs the source step and the no-grad target forward (AdaBN, :281-289); SAC mode refreshes the momentum
    teacher on every NET_MOMENTUM_ITER-th iteration of the epoch (`update_teacher = i % NET_MOMENTUM_ITER == 0`, :294), skips
    the source pass under TRAIN.TARGET_ONLY (:274-276).  Batches are what the reference's loaders yield, already on the device:
    (image, masks_gt) and (frames1, frames_gt, frames2, affine, affine_inv).  Returns the number of iterations.

    To watch the teacher's view consistency over a run (no labels needed), call `core.collect_consistency(True)` once and read
    `core.consistency_tables(reset=True)` at the logging interval from `on_iteration` (summarise_consistency, format_consistency):
    one more launch per target step."""
    n = 0
    for i, (batch_source, batch_target) in enumerate(zip(loader_source, loader_target)):
        if cfg_model.BASELINE:
            out = (baseline_train_iteration(net, optim, batch_source, batch_target[0]), None, None)
        else:
            update_teacher = i % cfg_model.NET_MOMENTUM_ITER == 0
            out = sac_train_iteration(net, optim, batch_source, batch_target, group_size, update_teacher, cfg_model.LR_TARGET,
                                      target_only=target_only)
        if on_iteration is not None:
            on_iteration(i, out)
        n = i + 1
    return n


def _dist_state(rank, world):
    import torch.distributed as dist
    on = dist.is_available() and dist.is_initialized()
    if world is None:
        world = dist.get_world_size() if on else 1
    if rank is None:
        rank = dist.get_rank() if on else 0
    return rank, world


def prep_batch(tensor, num_groups, group_size, rank=None, world=None, device=None, exchange="all_gather"):
    """Rank-local slice of one loaded target tensor [B, L, ...] (train.py:157-209).

    Every rank's loader delivers whole groups of L views.  With N*L/world >= L the groups stay where they were
    loaded: the result is just [B*L, ...].  Otherwise a group is spread over L/per consecutive ranks
    (per = N*L/world views each): rank r keeps views [f % L, f % L + per) of the first group loaded by rank
    f // L, f = r*per (the groups loaded by the other ranks are dropped, as in the reference).
    exchange="all_gather" moves the tensors exactly like train.py:194-195; "p2p" sends each rank only the `per`
    views it keeps (same result, 1/world of the bytes -- xGMI links are point-to-point anyway)."""
    import torch.distributed as dist
    rank, world = _dist_state(rank, world)
    assert (num_groups * group_size) % world == 0, "Batch size does not fit world size"
    per = num_groups * group_size // world
    if per >= group_size:
        if device is not None:
            tensor = tensor.to(device, non_blocking=True)
        return tensor.flatten(0, 1)
    assert tensor.size(1) == group_size, "Loaded sequence is incorrect {} vs. {}".format(tensor.size(1), group_size)
    # WHERE the exchange runs.  RCCL ("nccl") moves device tensors, stream-ordered: upload first, exchange on the device.  gloo
    # is a host transport: its collectives stage device tensors through pinned memory, but its send / recv hand the tensor's
    # data pointer to the TCP transport as it is -- with a device tensor the host reads (writes) VRAM through the PCIe BAR with
    # no ordering against the stream that fills (consumes) it.  Found by the 8-rank one-device test of round 6 (ranks that are
    # sender and receiver at once got torn slices).  With gloo the loader's HOST tensor is exchanged and only the `per` views
    # this rank keeps cross PCIe afterwards.
    host_exchange = dist.get_backend() == "gloo"
    if device is not None and not host_exchange:
        tensor = tensor.to(device, non_blocking=True)
    if host_exchange and tensor.is_cuda:
        tensor = tensor.cpu()
    first = rank * per
    owner, lo = first // group_size, first % group_size
    tensor = tensor.contiguous()
    if exchange == "all_gather":
        parts = [torch.empty_like(tensor) for _ in range(world)]
        dist.all_gather(parts, tensor)
        mine = parts[owner].flatten(0, 1)[lo:lo + per]
    else:
        assert exchange == "p2p", exchange
        flat = tensor.flatten(0, 1)
        mine = flat[lo:lo + per].clone() if owner == rank else torch.empty_like(flat[:per])
        work = []
        for dst in range(world):                    # what this rank owes the ranks whose slice lives here
            if dst != rank and (dst * per) // group_size == rank:
                d_lo = (dst * per) % group_size
                work.append(dist.P2POp(dist.isend, flat[d_lo:d_lo + per].contiguous(), dst))
        if owner != rank:
            work.append(dist.P2POp(dist.irecv, mine, owner))
        if work:
            for req in dist.batch_isend_irecv(work):
                req.wait()
    if device is not None and host_exchange:
        mine = mine.to(device, non_blocking=True)
    return mine


def sac_train_iteration(net, optim, src_batch, tgt_batch, group_size, update_teacher, lr_target, target_only=False,
                        sum_grads_in_optimizer=True, fuse_passes=False):
    """source fwd -> zero_grad -> source bwd (gradients kept) -> target fwd (teacher EMA first when asked)
    -> (LR_TARGET * self_ce) bwd -> one optimiser step.  Returns (source losses, target losses, net_outs)
    with the losses still on the device (no host sync here).  TRAIN.TARGET_ONLY skips the source pass altogether
    (train.py:274-276) and clears the gradients before the target backward (train.py:226-227).

    The reference lets autograd add the target-pass gradients onto the source-pass ones in `.grad` (320 `add_` launches for
    ResNet-101).  With a fused optimiser (`FusedSGD`, plain or Nesterov, and `FusedAdam`: anything that has `stash_grads`) the
    source gradients are set aside instead and the update kernel applies
    source + target -- on one rank the same sum, bit for bit.  Between the target backward and step(), and after it,
    `.grad` holds the target-pass gradient only: clipping and norm logging therefore happen inside the fused optimisers
    (`make_optimizer(..., max_grad_norm=, skip_nonfinite=)`, `optim.grad_norm`, `optim.measure_grad_norm()`: the norm of
    source + target, measured on the device; per tensor: `make_optimizer(..., tensor_stats=True)` and `gradient_report`); anything else that reads gradients before the step can use `optim.full_grads()`
    or pass sum_grads_in_optimizer=False (or another optimiser) for the reference's `.grad` contents.
    Under data parallelism the update is mean_r(src_r) + mean_r(tgt_r) where the reference's DDP reduces
    mean_r(mean(src) + tgt_r): equal in exact arithmetic, one rounding apart in fp32 (not bit-identical) -- for every fused
    optimiser alike.

    fuse_passes=True: the student runs ONCE over [source crops; target crops] and ONE backward pass differentiates
    loss_ce + LR_TARGET * self_ce (`SAC.forward_fused`: same weights in both passes, frozen BN, teacher independent of the
    student -- the same gradient sum, half the launches, one gradient all-reduce per iteration).  Needs the bare module or
    `dasac_hip.parallel.OverlappedDataParallel`; silently runs the two-pass order where it does not apply (target_only, stock
    DistributedDataParallel, batch-statistics BN, crops of different sizes, or a concatenated batch whose largest activation
    would leave the kernels' 4 GiB addressing window (FCN-8s at 16 crops of 512x1024 peaks at exactly 2 GiB: fused since round 5).

    View consistency: after `core.collect_consistency(True)` (once) every target step, fused or not, adds its groups to the
    label-free agreement tables -- one more launch per target step; read `core.consistency_tables(reset=True)` when logging."""
    core = _unwrap(net)
    if fuse_passes and not target_only and hasattr(net, "forward_fused") and hasattr(core, "backbone") and core.backbone._bn_frozen() \
            and tuple(src_batch[0].shape[1:]) == tuple(tgt_batch[0].shape[1:]) \
            and core.backbone._batch_fits(src_batch[0].shape[0] + tgt_batch[0].shape[0], *src_batch[0].shape[-2:]):
        images, masks = src_batch
        frames1, frames_gt, frames2, affine, affine_inv = tgt_batch
        losses_src, losses_tgt, outs = net.forward_fused(images, masks, frames1, frames_gt, frames2, affine, affine_inv,
                                                         update_teacher=update_teacher, T=group_size)
        optim.zero_grad()
        (losses_src["loss_ce"].mean() + lr_target * losses_tgt["self_ce"].mean()).backward()
        optim.step()
        return losses_src, losses_tgt, outs
    losses_src = {}
    if not target_only:
        images, masks = src_batch
        losses_src, _ = net(images, masks)
        optim.zero_grad()
        losses_src["loss_ce"].mean().backward()
        if sum_grads_in_optimizer and hasattr(optim, "stash_grads"):
            optim.stash_grads()
    frames1, frames_gt, frames2, affine, affine_inv = tgt_batch
    losses_tgt, outs = net(frames1, frames_gt, frames2, affine, affine_inv, use_teacher=True,
                           update_teacher=update_teacher, T=group_size)
    if target_only:
        optim.zero_grad()
    (lr_target * losses_tgt["self_ce"].mean()).backward()
    optim.step()
    return losses_src, losses_tgt, outs


def reduce_losses(losses, world=None):
    """train.py:243-246: every logged loss is summed over ranks and divided by the world size (one collective for the
    whole dict instead of one per key); returns python floats (the only host sync of a step)."""
    import torch.distributed as dist
    _, world = _dist_state(None, world)
    keys = sorted(losses)
    if not keys:
        return {}
    packed = torch.cat([losses[k].detach().reshape(-1)[:1] for k in keys])
    if world > 1:
        dist.all_reduce(packed)
        packed = packed / world
    return dict(zip(keys, packed.tolist()))


def baseline_train_iteration(net, optim, src_batch, tgt_images):
    """Baseline / AdaBN mode (train.py:274-289)."""
    images, masks = src_batch
    losses, _ = net(images, masks)
    optim.zero_grad()
    losses["loss_ce"].mean().backward()
    optim.step()
    with torch.no_grad():
        dummy = torch.zeros(tgt_images.shape[0], tgt_images.shape[2], tgt_images.shape[3], dtype=torch.int64, device=tgt_images.device)
        net(tgt_images, dummy)
    return losses


# --------------------------------------------------------------------------------------------------
# synthetic workload: weights, crops, labels and the four view affines
# --------------------------------------------------------------------------------------------------
def init_synthetic_weights(net, seed=0, classifier_gain=6.0):
    """Random-init weights of the right architecture, scaled like a trained network so that the
    reference's SGD hyper-parameters are stable: He-normal convs, BN gamma~U(.5,1.5), beta/mean~N(0,.1),
    var~U(.5,1.5); the BN that closes each residual branch x0.1 and the shortcut BN x0.3 keep the
    residual stream at E[f^2]~0.05-0.3 (full-range fp32 data, nothing zero-filled); classifier weights
    x6 give stride-8 logits of std~3 (peaked, unsaturated softmax: ~1/3 of the pseudo-labels fire)."""
    import torch.nn as nn
    gen = torch.Generator().manual_seed(seed)
    core = net.backbone if hasattr(net, "backbone") else net
    with torch.no_grad():
        for name, m in core.named_modules():
            if isinstance(m, nn.Conv2d):
                fan_in = m.in_channels * m.kernel_size[0] * m.kernel_size[1]
                w = torch.empty(m.weight.shape).normal_(0, (2.0 / fan_in) ** 0.5, generator=gen)
                if "conv2d_list" in name or name.startswith(("score_pool", "vgg_head.8")):
                    w *= classifier_gain
                m.weight.copy_(w)
                if m.bias is not None:
                    m.bias.copy_(torch.empty(m.bias.shape).normal_(0, 0.01, generator=gen))
            elif isinstance(m, (nn.SyncBatchNorm, nn.BatchNorm2d)):
                gain = 0.1 if name.endswith("bn3") else (0.3 if name.endswith("downsample.1") else 1.0)
                bgain = 0.3 if name.endswith("downsample.1") else 1.0
                m.weight.copy_(torch.empty(m.weight.shape).uniform_(0.5, 1.5, generator=gen) * gain)
                m.bias.copy_(torch.empty(m.bias.shape).normal_(0, 0.1, generator=gen) * bgain)
                m.running_mean.copy_(torch.empty(m.bias.shape).normal_(0, 0.1, generator=gen))
                m.running_var.copy_(torch.empty(m.bias.shape).uniform_(0.5, 1.5, generator=gen))
    return net


def view_affines(params, crop_h, crop_w):
    """theta / theta^-1 [L,2,3] of the augmented views, params = (dy, dx, alpha_deg, scale, flip) per view
    -- the formulas of /root/reference/datasets/dataloader_target.py:220-262."""
    import math
    L = len(params)
    theta = torch.zeros(L, 2, 3)
    ar = float(crop_h) / float(crop_w)
    for i, (dy, dx, alpha, scale, flip) in enumerate(params):
        s, c = math.sin(alpha * math.pi / 180.0), math.cos(alpha * math.pi / 180.0)
        theta[i, 0, 0], theta[i, 0, 1] = flip * c, s * ar
        theta[i, 1, 0], theta[i, 1, 1] = -s / ar, c
        theta[i, 0, 2] = -(c * dx + s * dy) / float(crop_w // 2)
        theta[i, 1, 2] = -(-s * dx + c * dy) / float(crop_h // 2)
        theta[i] *= scale
    inv = theta.clone()
    inv[:, 0, 1] = theta[:, 1, 0] * ar ** 2
    inv[:, 1, 0] = theta[:, 0, 1] / ar ** 2
    inv[:, 0, 2] = -(inv[:, 0, 0] * theta[:, 0, 2] + inv[:, 0, 1] * theta[:, 1, 2])
    inv[:, 1, 2] = -(inv[:, 1, 0] * theta[:, 0, 2] + inv[:, 1, 1] * theta[:, 1, 2])
    inv /= torch.tensor([p[3] for p in params], dtype=torch.float32).view(-1, 1, 1) ** 2
    return theta, inv


# identity | zoom .7 + shift + flip | zoom .5 + shift | flip only   
BENCH_VIEWS = [(0.0, 0.0, 0.0, 1.0, 1.0), (40.0, -100.0, 0.0, 0.7, -1.0), (-60.0, 30.0, 0.0, 0.5, 1.0), (0.0, 0.0, 0.0, 1.0, -1.0)]


def synthetic_batches(batch, groups, views, size, device, seed=0, num_classes=19):
    """(source batch, target batch) of the cfg-3 shape: N(0,1) crops, random labels with a 16-px ignore
    border, target labels with 3 padded (-1) rows, frames2 = frames1 + 0.01*noise."""
    H, W = size
    gen = torch.Generator().manual_seed(seed)
    xs = torch.randn(batch, 3, H, W, generator=gen)
    ys = torch.randint(0, num_classes, (batch, H, W), generator=gen)
    ys[:, :16] = 255
    ys[:, -16:] = 255
    ys[:, :, :16] = 255
    ys[:, :, -16:] = 255
    B = groups * views
    f1 = torch.randn(B, 3, H, W, generator=gen)
    f2 = f1 + 0.01 * torch.randn(B, 3, H, W, generator=gen)
    gt = torch.randint(0, num_classes, (B, H, W), generator=gen)
    gt[:, :3] = -1
    sc = min(H, W) / 769.0
    params = [(dy * sc, dx * sc, a, s, f) for (dy, dx, a, s, f) in BENCH_VIEWS[:views]]
    theta, inv = view_affines(params, H, W)
    to = lambda t: t.to(device)
    return (to(xs), to(ys)), (to(f1), to(gt), to(f2), to(theta.repeat(groups, 1, 1)), to(inv.repeat(groups, 1, 1)))


def self_consistent_labels(net, images, border=16):
    """Source labels = the freshly initialised network's own argmax (with the ignore border): a
    converged-model regime, so that the reference's SGD hyper-parameters (LR 2.5e-4, x10 on the
    classifier, LR_TARGET 5) stay numerically stable on synthetic data for any number of steps."""
    core = net.backbone if hasattr(net, "backbone") else net
    with eval_mode(core), torch.no_grad():
        ys = torch.cat([core(images[i:i + 1])[1].argmax(1) for i in range(images.shape[0])], 0)
    ys[:, :border] = 255
    ys[:, -border:] = 255
    ys[:, :, :border] = 255
    ys[:, :, -border:] = 255
    return ys


def _classifier_layers(core):
    import torch.nn as nn
    return [m for n, m in core.named_modules()
            if isinstance(m, nn.Conv2d) and ("conv2d_list" in n or n.startswith(("score_pool", "vgg_head.8")))]


def calibrate_classifier(net, image, target_std=3.0):
    """Rescales the (linear) classifier layers of a synthetic-weight net so that its stride-8 logits have the given
    standard deviation on `image` -- peaked but unsaturated softmax whatever the backbone's feature scale is."""
    core = net.backbone if hasattr(net, "backbone") else net
    with eval_mode(core), torch.no_grad():
        std = float(core(image)[0].std())
        f = target_std / max(std, 1e-12)
        for m in _classifier_layers(core):
            m.weight.mul_(f)
            if m.bias is not None:
                m.bias.mul_(f)
    return f


# --------------------------------------------------------------------------------------------------
# checkpoints and validation
# --------------------------------------------------------------------------------------------------
def save_checkpoint(path, net, optim, score, epoch):
    """File layout of the reference's utils/checkpoints.py:62-74: {"model": state dict with the DDP
    "module." prefix, "opt": optimiser state, "score", "epoch"}."""
    core = _unwrap(net)
    model = {"module." + k: v for k, v in core.state_dict().items()}
    torch.save({"model": model, "opt": optim.state_dict() if optim is not None else None, "score": score, "epoch": epoch}, path)


def load_checkpoint(path, net, optim=None, map_location="cpu"):
    """utils/checkpoints.py:49-60: strict=False, so a baseline snapshot (backbone only) loads into SAC and
    leaves the teacher / class prior to the first `_momentum_update`.  Accepts keys with or without "module."."""
    blob = torch.load(path, map_location=map_location)
    core = _unwrap(net)
    model = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in blob["model"].items()}
    missing, unexpected = core.load_state_dict(model, strict=False)
    if optim is not None and blob.get("opt") is not None:
        optim.load_state_dict(blob["opt"])
    return blob.get("epoch", 0), blob.get("score", 0.0), missing, unexpected


# Cityscapes train id -> label id (cityscapesScripts `labels`; what infer_val.py:60-65 `convert_to_cs` applies)
CITYSCAPES_TRAIN_TO_ID = (7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33)


def _infer_backbone_and_lut(net, image, lut, teacher):
    """What both inference paths start from: the network that gives the logits (the unwrapped net itself, or SAC's student
    backbone / `slow_net` teacher) and `lut` as a uint8 tensor on the image's device (or None)."""
    core = _unwrap(net)
    backbone = core
    if hasattr(core, "backbone"):
        backbone = core.slow_net if teacher else core.backbone
    if lut is not None and not torch.is_tensor(lut):
        lut = torch.tensor(list(lut), dtype=torch.uint8, device=image.device)
    return backbone, lut


def infer_label_maps(net, image, lut=None, teacher=False, want_conf=False):
    """infer_val.py:160-163 + the writer's argmax / id mapping, without materialising logits_up or the softmax:
    backbone -> low-resolution logits -> ONE kernel -> uint8 label map [B,H,W] on the device (PNG writing stays on
    the host).  `lut`: uint8 tensor / sequence (e.g. CITYSCAPES_TRAIN_TO_ID) or None for train ids."""
    from dasac_hip import ops
    backbone, lut = _infer_backbone_and_lut(net, image, lut, teacher)
    with torch.no_grad():
        logits = backbone._logits(image)
        return ops.infer_labels(logits, image.shape[-2:], lut, want_conf)


INFER_MS_MAX_SOURCES = 8                     # ops.INFER_MAX_SOURCES: what one infer_fuse launch takes


def scaled_size(H, W, scale):
    """The size rule of the multi-scale path: (int(H * s + 0.5), int(W * s + 0.5))."""
    return int(H * scale + 0.5), int(W * scale + 0.5)


def _ms_plan(H, W, scales, flip):
    """[(Hs, Ws, needs_pyramid)] per scale; ValueError for no scale, too many sources or a scale that leaves no pixel."""
    scales = tuple(float(s) for s in scales)
    if not scales:
        raise ValueError("infer_label_maps_ms: no scale given")
    n_sources = len(scales) * (2 if flip else 1)
    if n_sources > INFER_MS_MAX_SOURCES:
        raise ValueError("infer_label_maps_ms: {} scales{} make {} sources; one launch takes {}".format(
            len(scales), " x 2 orientations" if flip else "", n_sources, INFER_MS_MAX_SOURCES))
    plan = []
    for s in scales:
        Hs, Ws = scaled_size(H, W, s)
        if Hs < 1 or Ws < 1:
            raise ValueError("infer_label_maps_ms: scale {} of a {}x{} image gives {}x{}".format(s, H, W, Hs, Ws))
        plan.append((Hs, Ws, flip or s != 1.0))
    return plan


def crf_refine(probs, image, params, lut=None, want_conf=False, want_probs=False):
    """Mean-field CRF refinement (crf.CrfParams; include/dasac_hip.h: dasac_crf_meanfield) of class probabilities fp32 [B,C,H,W] --
    what infer_label_maps_ms(..., want_probs=True) returns -- over the image fp32 [B,Ci,H,W] the network saw.  Returns (labels u8
    [B,H,W] through `lut` if given, conf f32 [B,H,W] or None, probs f32 [B,C,H,W] or None) of the refined distribution.  One launch
    per iteration; torch only allocates."""
    from dasac_hip import ops
    if lut is not None and not torch.is_tensor(lut):
        lut = torch.tensor(list(lut), dtype=torch.uint8, device=probs.device)
    return ops.crf_meanfield(probs, image, params, lut, want_conf, want_probs)


def infer_label_maps_ms(net, image, scales=(0.5, 0.75, 1.0), flip=True, mode="mean", lut=None, teacher=False, want_conf=False,
                        want_probs=False, crf=None):
    """infer_label_maps with test-time augmentation: the image at every scale of `scales`, plain and (with `flip`) mirrored, the
    class probabilities of all of them fused by mean or max (`mode`) at the image's own size.  Per scale s the backbone sees
    scaled_size(H, W, s) pixels: ONE ops.image_pyramid launch makes the scaled (and mirrored) input -- none for s == 1.0 without
    flip, the image itself is passed -- and ONE `_logits` call runs it, at batch 2B when flipping; then ONE ops.infer_fuse launch
    over all the halves (the mirrored half is a batch slice of the same logits tensor) writes the uint8 label map.  No
    upsampled, flipped, softmaxed or summed [B,C,H,W] tensor exists; torch only allocates.  At most 8 sources (scales x
    orientations).  Returns (labels u8 [B,H,W], conf f32 [B,H,W] or None, probs f32 [B,C,H,W] or None): conf is the winning fused
    probability, probs all of them (infer_val.py's D_SAVE_RAW).  `lut`, `teacher` as infer_label_maps.
    With `crf` (a crf.CrfParams) the fused probabilities go through crf_refine over `image` -- the step DeepLabv2's published
    pipeline ends in -- and labels, conf and probs are those of the refined distribution; infer_fuse's own label map is discarded.
    None (the default) leaves the call launch for launch what it is without the argument."""
    from dasac_hip import ops
    B, _, H, W = image.shape
    plan = _ms_plan(H, W, scales, flip)
    backbone, lut = _infer_backbone_and_lut(net, image, lut, teacher)
    sources, flips = [], []
    with torch.no_grad():
        for Hs, Ws, resample in plan:
            logits = backbone._logits(ops.image_pyramid(image, (Hs, Ws), flip) if resample else image)
            sources.append(logits[:B])
            flips.append(False)
            if flip:
                sources.append(logits[B:])
                flips.append(True)
        if crf is None:
            return ops.infer_fuse(sources, flips, (H, W), mode, lut, want_conf, want_probs)
        _, _, probs = ops.infer_fuse(sources, flips, (H, W), mode, None, False, True)
        return crf_refine(probs, image, crf, lut, want_conf, want_probs)


def validation_iou(net, batches, num_classes=19, scales=None, flip=False, confusion=False, boundary_radius=0, crf=None):
    """mIoU over (image, label) batches: argmax + per-class tp/fp/fn in one kernel pass per batch
    (train.py:339-469, utils/metrics.py:9-53); counts are all-reduced when a process group exists.
    With `scales` (or `flip`) the prediction is infer_label_maps_ms's label map (scales defaults to (1.0,) when only `flip` is
    set) and the counts come from the label-layer counter (ops.mask_counts, as `validation` counts `teacher_labels`); the uint8
    map is widened to the int64 that counter reads, the one torch operation of that path.
    With `confusion` the pass is ops.confusion_counts instead -- it reads the uint8 map as it is -- the counts follow from the
    matrix (counts_from_confusion: the same integers) and the return value is (mIoU, iou, matrix int64 [C+1,C+1] on the host: row =
    ground truth, column = prediction, index C = no class; see summarise_confusion).
    With `boundary_radius` R > 0 one ops.boundary_counts per batch runs beside that pass on the same prediction, and the return value
    gains a last element: the boundary table int64 [R+1,5,C] on the host, summed over ranks (summarise_boundary reads
    {"prediction": table}).  0 changes nothing.
    With `crf` (a crf.CrfParams) the prediction is the CRF-refined map of infer_label_maps_ms(..., crf=crf): it implies that path
    (scales (1.0,) if none is given), and the counters and the boundary table read the refined maps."""
    from dasac_hip import ops
    core = _unwrap(net)
    counts, boundary, radius = None, None, int(boundary_radius)
    multi_scale = scales is not None or flip or crf is not None
    with eval_mode(core), torch.no_grad():
        for image, gt in batches:
            if multi_scale:
                maps, _, _ = infer_label_maps_ms(net, image, (1.0,) if scales is None else scales, flip, crf=crf)
                if confusion:
                    counts, _ = ops.confusion_counts([], [maps], gt, counts, num_classes=num_classes)
                else:
                    counts = ops.mask_counts([], [maps.to(torch.int64)], gt, counts, num_classes=num_classes)
                if radius > 0:
                    boundary = ops.boundary_counts([], [maps], gt, boundary, radius, num_classes=num_classes)
            else:
                _, logits_up = core(image)
                if confusion:
                    counts, _ = ops.confusion_counts([logits_up], [], gt, counts)
                else:
                    counts = ops.iou_counts(logits_up, gt, counts)
                if radius > 0:
                    boundary = ops.boundary_counts([logits_up], [], gt, boundary, radius)
    if (multi_scale or confusion) and counts is not None:
        counts = counts[0]
    counts = rank_sum(counts)
    if boundary is not None:
        boundary = rank_sum(boundary)
    matrix = counts.cpu() if confusion else None
    iou, _, _ = summarise_iou(counts_from_confusion(matrix) if confusion else counts)
    result = (float(iou.mean()), iou, matrix) if confusion else (float(iou.mean()), iou)
    return result + (boundary[0].cpu(),) if radius > 0 and boundary is not None else result


# --------------------------------------------------------------------------------------------------
# activation tables: per-layer activation health and the source / target domain gap (no counterpart in the reference)
# --------------------------------------------------------------------------------------------------
class ActivationRecord:
    """One probed engine forward: net ("backbone" / "slow_net"), N (batch size), bounds (the full segment tuple (0, ..., N)),
    table (device fp64 [n_segments, R, 6], dasac_hip.ops.ACTIVATION_STATS_COLUMNS) and layout (`Engine.activation_layout`)."""

    def __init__(self, net, N, bounds, table, layout):
        self.net, self.N, self.bounds, self.table, self.layout = net, int(N), tuple(bounds), table, layout

    def __repr__(self):
        return "ActivationRecord(net={!r}, N={}, bounds={}, layers={})".format(self.net, self.N, self.bounds, len(self.layout))


class ActivationProbe:
    """What `activation_probe` yields: `passes` lists one ActivationRecord per engine forward inside the block, in call order."""

    def __init__(self, bounds=None):
        self.bounds, self.passes = bounds, []


class _ProbeTap:
    """The probe as one engine sees it (Engine.forward): the shared bounds, this net's module names, records tagged with its net."""

    def __init__(self, probe, net, names):
        self.probe, self.net, self.names = probe, net, names

    @property
    def bounds(self):
        return self.probe.bounds

    def append(self, item):
        table, layout, N, bounds = item
        self.probe.passes.append(ActivationRecord(self.net, N, bounds, table, layout))


def _probed_nets(net):
    core = _unwrap(net)
    nets = [("backbone", core.backbone if hasattr(core, "backbone") else core)]
    if hasattr(core, "slow_net"):
        nets.append(("slow_net", core.slow_net))
    return nets


class activation_probe:
    """Context manager: per-layer activation tables of every backbone forward inside the block.

        with driver.activation_probe(net, bounds=(n_src,)) as probe:
            driver.sac_train_iteration(net, optim, src, tgt, T, update, lr_target, fuse_passes=True)
        report = driver.domain_gap_report(probe.passes[-1])           # the student over [source; target]

    Attaches one probe to the engines of `backbone` and, for SAC, `slow_net` (through `.module` of a DistributedDataParallel /
    OverlappedDataParallel wrapper) and detaches it on exit.  While attached, every engine forward keeps all its activations
    until its end (a no-grad pass then needs the memory of a training pass) and adds one dasac_activation_stats call: two launches,
    no synchronisation, no ATen arithmetic; losses, logits and gradients are bit for bit what they are without it.  `probe.passes`:
    one ActivationRecord per forward, in call order (a two-pass SAC iteration: student source, student target, teacher; with
    fuse_passes: teacher, student over the concatenated batch).
    bounds: None (one segment), the interior cut points of the batch ((n_src,)), or a callable N -> bounds for passes of different
    sizes.  Replacing a module's Parameter objects inside the block (which re-captures the engine) drops the probe.
    Tables are PER RANK: columns sum, sumsq, nonfinite and zeros add across ranks, maxabs takes the maximum, and first_nonfinite
    is an index into the rank's own batch -- reduce them yourself where a global view is wanted."""

    def __init__(self, net, bounds=None):
        self.net, self.probe, self._engines = net, ActivationProbe(bounds), []

    def __enter__(self):
        from dasac_hip import engine as E
        for tag, sub in _probed_nets(self.net):
            if sub._engine is None or sub._engine.stale():
                sub._engine = E.Engine(sub._plan())
            if sub._engine.probe is not None:
                self.__exit__()
                raise RuntimeError("activation_probe: {} already has a probe attached".format(tag))
            sub._engine.probe = _ProbeTap(self.probe, tag, {m: name for name, m in sub.named_modules()})
            self._engines.append(sub._engine)
        return self.probe

    def __exit__(self, *exc):
        for eng in self._engines:
            eng.probe = None
        self._engines = []
        return False


def activation_stats(net, images, bounds=None, teacher=False):
    """The stand-alone form: one no-grad forward of the student backbone (teacher=True: the momentum teacher) over `images`
    [N,3,H,W] with a probe attached; returns its ActivationRecord.  bounds as in `activation_probe`."""
    nets = dict(_probed_nets(net))
    with torch.no_grad(), activation_probe(net, bounds) as probe:
        nets["slow_net" if teacher else "backbone"](images)
    assert len(probe.passes) == 1
    return probe.passes[0]


# --------------------------------------------------------------------------------------------------
# class-conditional feature tables: per-class prototypes of one activation and the per-class domain gap (no counterpart in the
# reference)
# --------------------------------------------------------------------------------------------------
class ClassFeatureRecord:
    """What `class_features` returns: table (dasac_hip.ops.ClassFeatureTable: sums fp64 [C,Cf,2], counts int64 [C], on the device),
    layer (the resolved name of the tapped activation), Cf, radius, labels ("given" / "prediction"), num_classes, net ("backbone" /
    "slow_net") and batches (how many went in)."""

    def __init__(self, table, layer, Cf, radius, labels, num_classes, net, batches=0):
        self.table, self.layer, self.Cf, self.radius, self.labels = table, layer, int(Cf), int(radius), labels
        self.num_classes, self.net, self.batches = int(num_classes), net, int(batches)

    def __repr__(self):
        return "ClassFeatureRecord(net={!r}, layer={!r}, Cf={}, C={}, radius={}, labels={!r}, batches={})".format(
            self.net, self.layer, self.Cf, self.num_classes, self.radius, self.labels, self.batches)


def class_features(net, batches, labels="given", layer=None, radius=2, num_classes=19, teacher=False, into=None):
    """Per-class, per-channel moments of ONE activation of the backbone, accumulated over `batches` on the device.

        src = driver.class_features(net, source_batches)                                   # ground truth
        tgt = driver.class_features(net, target_batches, labels="prediction")              # no ground truth needed
        print(driver.format_class_gap_report(driver.class_gap_report(src, tgt), class_names))

    batches yields (image [B,3,H,W], label map [B,H,W] int64 / uint8 or None), on the device.  Per batch: one no-grad forward of
    the student backbone (teacher=True: `slow_net`) with an engine tap on `layer` (a name of `Engine.activation_layout`; None: the
    classifier's input, see `Engine.tap_index`), one ops.label_nodes launch that brings the label map to the activation's
    resolution (a node keeps its class only if the whole (2 radius + 1)^2 window around its pixel holds it) and one
    ops.class_feature_stats launch.  labels="given" takes the map as it is (ground truth, or the `teacher_labels` of a target
    step); labels="prediction" takes the arg-max of that same forward's logits at the image's resolution (ops.infer_labels), so
    the window speaks of predicted regions.  Eval mode, restored afterwards; teacher, class prior and optimiser are untouched.
    The tap is detached after every forward, also when it fails.  `into`: a record to continue; a different net, layer, Cf,
    radius, label source or class count is refused.  Tables are PER RANK: see `reduce_class_features`."""
    from dasac_hip import engine as E
    from dasac_hip import ops
    if labels not in ("given", "prediction"):
        raise ValueError("class_features: labels is \"given\" or \"prediction\" (got {!r})".format(labels))
    core = _unwrap(net)
    backbone, _ = _infer_backbone_and_lut(net, None, None, teacher)
    tag = "slow_net" if (teacher and hasattr(core, "backbone")) else "backbone"
    radius, num_classes = int(radius), int(num_classes)
    record, eng = into, None
    with eval_mode(core), torch.no_grad():
        for image, label_map in batches:
            if backbone._engine is None or backbone._engine.stale():
                backbone._engine = E.Engine(backbone._plan())
            if backbone._engine is not eng:               # once per engine: the first batch, or parameters replaced in between
                eng = backbone._engine
                index, name = eng.tap_index(layer, {m: n for n, m in backbone.named_modules()})
            if eng.tap is not None:
                raise RuntimeError("class_features: the engine of {} already has a tap attached".format(tag))
            got = []
            eng.tap = (index, got.append)
            try:
                logits = backbone._logits(image)
            finally:
                eng.tap = None
            feat = got[0]
            if record is None:
                record = ClassFeatureRecord(ops.ClassFeatureTable.zeros(num_classes, feat.shape[1], feat.device), name, feat.shape[1],
                                            radius, labels, num_classes, tag)
            elif (record.net, record.layer, record.Cf, record.radius, record.labels, record.num_classes) != \
                    (tag, name, int(feat.shape[1]), radius, labels, num_classes):
                raise ValueError("class_features: {!r} cannot take net={!r}, layer={!r}, Cf={}, radius={}, labels={!r}, C={}".format(
                    record, tag, name, int(feat.shape[1]), radius, labels, num_classes))
            if labels == "prediction":
                label_map, _ = ops.infer_labels(logits, image.shape[-2:])
            elif label_map is None:
                raise ValueError("class_features: labels=\"given\" needs a label map with every batch")
            nodes = ops.label_nodes(label_map, feat.shape[-2:], num_classes, radius)
            ops.class_feature_stats(feat, nodes, num_classes, record.table)
            record.batches += 1
    if record is None:
        raise ValueError("class_features: no batches")
    return record


def reduce_class_features(record):
    """Sums a record's table over the ranks of the process group, in place: one collective for `sums`, one for `counts` (both
    add).  gloo moves device tensors with no ordering against the stream that fills them (see prep_batch), so under gloo the HOST
    tensors are summed and the record then holds host tensors; RCCL sums on the device.  Without a process group (or with one
    rank) nothing happens.  Returns the record."""
    sums, counts = rank_sum(record.table.sums), rank_sum(record.table.counts)
    if sums is not record.table.sums:                     # gloo: the sums are host copies
        record.table = type(record.table)(sums, counts)
    return record


def compute_sample_weights(net, batches, num_images, lut=None, teacher=False, scales=None, flip=False):
    """Stage 2 of the reference's schedule (tools/compute_IS_weights.py on the masks infer_val.py wrote) without leaving the
    device: per-image class pixel counts of the network's label maps, int64 [num_images,256] on the host -- the input of
    sampling.weights_from_counts.  `batches` yields (image [B,3,H,W] on the device, global image indices [B] as a HOST
    sequence / tensor); each batch is infer_label_maps -> ops.label_hist into the rows of one device table, one launch per
    run of consecutive indices, with no host synchronisation inside the loop and one D2H copy at the end.  The network runs
    in eval mode.  With a process group of world > 1 each rank passes its own slice of the images and the tables are summed
    over ranks; a row no rank touched stays zero.  `lut` as infer_label_maps (e.g. CITYSCAPES_TRAIN_TO_ID: the counts land
    in the Cityscapes-id bins).  With `scales` (or `flip`) the label maps are infer_label_maps_ms's (scales defaults to (1.0,)
    when only `flip` is set)."""
    from dasac_hip import ops
    core = _unwrap(net)
    table = torch.zeros((num_images, 256), dtype=torch.int64, device=next(core.parameters()).device)
    with eval_mode(core):
        for image, index in batches:
            index = [int(i) for i in (index.tolist() if torch.is_tensor(index) else index)]
            assert len(index) == image.shape[0] and all(0 <= i < num_images for i in index), (index, num_images)
            if scales is not None or flip:
                maps = infer_label_maps_ms(net, image, (1.0,) if scales is None else scales, flip, lut=lut, teacher=teacher)[0]
            else:
                maps, _ = infer_label_maps(net, image, lut, teacher)
            lo = 0
            for hi in range(1, len(index) + 1):
                if hi == len(index) or index[hi] != index[hi - 1] + 1:
                    ops.label_hist(maps[lo:hi], table[index[lo]:index[lo] + hi - lo])
                    lo = hi
    return rank_sum(table).cpu()                          # summed on the device under RCCL, before the one D2H copy


# --------------------------------------------------------------------------------------------------
# reference-form validation (train.py:339-469): student and teacher IoU, loss means, checkpoint score
# --------------------------------------------------------------------------------------------------
VALIDATION_SCORE_LAYERS = ("logits_up", "teacher_init", "teacher_refined")      # through argmax(., 1), train.py:394-395
VALIDATION_LABEL_LAYERS = ("teacher_labels",)                                   # label maps as they are, 255 = no label (:396-397)
VALIDATION_LOGITS_LAYERS = ("logits_up", "teacher_init")                        # logits; `teacher_refined` holds probabilities


def validation_batches(loader, max_iter=None):
    """The batches `Trainer.validation` evaluates (train.py:347-348,375,405-406): `max_iter` defaults to len(loader), and the
    loop leaves on `n > max_iter` AFTER it has processed batch n -- a longer loader contributes max_iter + 2 batches."""
    if max_iter is None and hasattr(loader, "__len__"):
        max_iter = len(loader)
    for n, batch in enumerate(loader):
        yield batch
        if max_iter is not None and n > max_iter:
            break


def _step_inputs(batch, step, group_size, num_groups, device, world):
    """What the forward pass of `validation` / `visualise_results` takes for one loaded batch, on the device: the positional tensors
    ((image, gt), or the five target tensors through `prep_batch`) and the keyword arguments of the step (train=False)."""
    if step == "source":
        return [t.to(device, non_blocking=True) for t in batch[:2]], {}
    groups = num_groups if num_groups is not None else batch[0].shape[0] * world
    return [prep_batch(t, groups, group_size, device=device) for t in batch], dict(use_teacher=True, update_teacher=False, T=group_size)


def validation(net, loader, step="source", group_size=None, max_iter=None, ignore_classes=(), num_classes=19, num_groups=None,
               confusion=False, reliability_bins=0, consistency=False, consistency_cover=0.5, boundary_radius=0, segment_tables=False,
               segment_connectivity=8):
    """`Trainer.validation` (train.py:339-469) with its step function (`step` :119-155 or `_step_target` :211-250, train=False):
    eval mode under no_grad (the previous mode is restored), loss means, one (tp, fp, fn) table per mask layer, the per-class and
    class-subset summaries and the checkpoint score.  Neither the teacher nor the class prior is updated.

      step="source": batches (image, gt); `net(image, gt)`; the layer is `logits_up`; losses are THIS rank's `val.mean()`
                     (train.py:147-151, no reduction over ranks).  A baseline net validates its target set this way (:113-115).
      step="target": batches (frames1, frames_gt, frames2, affine, affine_inv) as loaded, [N,T,...] each, through `prep_batch`
                     (`num_groups` defaults to loaded groups x world); `net(f1, gt, f2, affine, affine_inv, use_teacher=True,
                     update_teacher=False, T=group_size)`; layers `logits_up`, `teacher_init`, `teacher_refined` (arg-max) and
                     `teacher_labels` (as it is) against the frames_gt the forward pass has rewritten from -1 to 255; losses are
                     averaged over ranks (:243-246: fp32 sum over ranks / world per batch -- here ONE collective over the
                     [batches, keys] matrix after the loop, the same arithmetic as `reduce_losses`; every rank must see the
                     same number of batches, as in the reference).

    All layers of a batch go through ONE `ops.mask_counts` launch into one device table; nothing in the loop waits for the
    device beyond what the forward pass does; one D2H copy at the end.  With a process group of world > 1 the tables are summed
    over ranks (gloo: the HOST table, see rank_sum; RCCL: on the device).  `max_iter`: see validation_batches.
    Loss means follow StatManager (stat_mean).  Returns a namespace: losses {key: mean}, counts {layer: int64 [3,C]}, per_class
    {layer: (jaccard, precision, recall)}, mean {layer: (mIoU, precision, recall)} over the classes not in `ignore_classes`,
    checkpoint_score = max over layers of mIoU.  The reference computes the score on its main process only and returns 0.0
    elsewhere; here EVERY rank returns the same value (each holds the summed counts) -- save on rank 0 only as before.
    Not reproduced: metrics.py:30 overwrites the prediction in place at ignored pixels (nothing reads it afterwards), and the
    reference's float32 counters, which stop being exact past 2^24 pixels per class -- the counts here are exact int64.

    Beyond the reference, opt-in: with `confusion` or `reliability_bins` > 0 the one launch per batch is `ops.confusion_counts`
    instead, and the namespace's `confusion` {layer: int64 [C+1,C+1]} (row = ground truth, column = prediction, index C = no class:
    summarise_confusion, pseudo_label_audit, format_confusion) and, with bins, `reliability` {score layer: int64 [C,bins,2]}
    (arg-max class, confidence bin, miss / hit: summarise_reliability; `logits_up` and `teacher_init` are binned by their soft-max
    maximum, `teacher_refined` by its winning probability) are filled; both are empty dicts otherwise.  `counts` then follows from
    the matrices (counts_from_confusion) and holds the same integers, so every other field is unchanged.  The tables share one
    device buffer: they are summed over ranks and copied to the host as `table` is, once.

    Label-free, opt-in, step="target" only (ValueError otherwise): with `consistency` the pass switches the model's
    view-consistency collection on (`SAC.collect_consistency`, coverage threshold `consistency_cover`) on a fresh accumulator --
    one more launch per batch, ops.view_consistency on the T aligned teacher views -- and restores the model's previous switch
    and accumulator afterwards.  The namespace's `consistency` is {"agree": int64 [C+1,T+1,T+1], "flips": [C,C], "per_view":
    [T,2]} on the host, summed over ranks as `table` is (one buffer, one collective, one copy), and `consistency_summary` is
    summarise_consistency of it (format_consistency renders it); {} and None when off.  Reported only: no other field, the
    checkpoint score included, depends on it.

    Where in the image the errors are, opt-in: with `boundary_radius` R > 0 (at most ops.BOUNDARY_MAX_RADIUS) one
    ops.boundary_counts per batch runs beside the count pass on the same layers into one device table, which is summed over ranks
    as `table` is and copied once.  The namespace's `boundary` is {layer: int64 [R+1,5,C]} on the host (slot = Chebyshev distance to
    the nearest class contour - 1, the last slot everything further; rows tp, fp, fn, pred, both) and `boundary_summary` is
    summarise_boundary of it at the radii 1, 2, 4, ... up to R: trimap-band, interior and Boundary IoU per class and layer
    (format_boundary renders it); {} and None when off.  Reported only: every other field is the one of a run without it.

    On which objects the errors are, opt-in: with `segment_tables` one ops.segment_counts per batch runs beside the count pass on
    the same layers (connected components under `segment_connectivity` 4 or 8) into one device table, which is summed over ranks
    as `table` is -- its collective comes last -- and copied once.  The namespace's `segments` is {layer: int64 [2,24,4,C]} on the
    host (side 0 the ground truth's segments, side 1 the predicted map's; bin floor(log2(size)); rows ops.SEGMENT_ROWS) and
    `segment_summary` is summarise_segments of it: object recall, segment precision and fragmentation per size group and class
    (format_segments renders it); {} and None when off.  Reported only: every other field is the one of a run without it."""
    from types import SimpleNamespace
    from dasac_hip import ops
    assert step in ("source", "target"), step
    if consistency and step != "target":
        raise ValueError("validation: view consistency needs the teacher's aligned views, step='target' (got step={!r})".format(step))
    core = _unwrap(net)
    if consistency and not hasattr(core, "swap_consistency"):
        raise ValueError("validation: {} collects no view consistency".format(type(core).__name__))
    device = next(core.parameters()).device
    _, world = _dist_state(None, None)
    joint, bins = bool(confusion) or int(reliability_bins) > 0, int(reliability_bins)
    layers, table, rows, keys, matrices, rel = None, None, [], None, None, None
    cons, cons_was = None, None
    radius, bound = int(boundary_radius), None
    seg = None
    if consistency:
        cons_was = core.swap_consistency((True, consistency_cover, None))
    try:
        with eval_mode(core), torch.no_grad():
            for batch in validation_batches(loader, max_iter):
                inputs, kw = _step_inputs(batch, step, group_size, num_groups, device, world)
                losses, outs = net(*inputs, **kw)
                gt = inputs[1].view(-1, *inputs[1].shape[-2:])
                if layers is None:
                    layers = ([k for k in VALIDATION_SCORE_LAYERS if k in outs], [k for k in VALIDATION_LABEL_LAYERS if k in outs])
                    keys = sorted(losses)
                scores, maps = [outs[k] for k in layers[0]], [outs[k] for k in layers[1]]
                if consistency and scores[0].shape[1] != num_classes:
                    # on EVERY rank, before any collective: a rank that owns no group sizes its zero tables from num_classes
                    raise ValueError("validation: num_classes={} but the net has {} classes: the consistency tables of the ranks "
                                     "would differ in size".format(num_classes, scores[0].shape[1]))
                if joint:
                    if table is None:               # one buffer: [L][C+1][C+1] matrices, then [Ls][C][bins][2] reliability tables
                        n_mat, side = len(scores) + len(maps), num_classes + 1
                        table = torch.zeros(n_mat * side * side + len(scores) * num_classes * bins * 2, dtype=torch.int64, device=device)
                        matrices = table[:n_mat * side * side].view(n_mat, side, side)
                        rel = table[n_mat * side * side:].view(len(scores), num_classes, bins, 2) if bins > 0 else None
                    logits = [i for i, k in enumerate(layers[0]) if k in VALIDATION_LOGITS_LAYERS]
                    ops.confusion_counts(scores, maps, gt, matrices, rel, logits_layers=logits)
                else:
                    table = ops.mask_counts(scores, maps, gt, table, num_classes=num_classes)
                if radius > 0:
                    bound = ops.boundary_counts(scores, maps, gt, bound, radius, num_classes=num_classes)
                if segment_tables:
                    seg = ops.segment_counts(scores, maps, gt, seg, segment_connectivity, num_classes=num_classes)
                rows.append(torch.cat([losses[k].detach().mean().reshape(1) for k in keys]))
    finally:
        if consistency:
            cons = core.swap_consistency(cons_was)[2]
    if table is None:
        return SimpleNamespace(losses={}, counts={}, per_class={}, mean={}, checkpoint_score=0.0, confusion={}, reliability={},
                               consistency={}, consistency_summary=None, boundary={}, boundary_summary=None, segments={},
                               segment_summary=None)
    if consistency and cons is None:        # a rank that owns no group (views sharded over ranks) still takes part in the sum
        cons = ops.consistency_tables(num_classes, group_size, device)
    names = layers[0] + layers[1]
    loss_rows = torch.stack(rows)
    # the collectives, in the one order every rank follows: counts, loss rows, consistency, boundary, segments (rank_sum: nothing on
    # one rank)
    table = rank_sum(table)
    if step == "target" and world > 1:
        loss_rows = rank_sum(loss_rows) / world
    if consistency:
        cons = ops.ConsistencyTables(rank_sum(cons.buffer), cons.C, cons.T)
    if bound is not None:
        bound = rank_sum(bound)
    if seg is not None:
        seg = rank_sum(seg)
    table, loss_rows = table.cpu(), loss_rows.cpu().tolist()
    bound_tables, bound_summary = {}, None
    if bound is not None:
        bound = bound.cpu()
        bound_tables = {name: bound[i] for i, name in enumerate(names)}
        bound_summary = summarise_boundary(bound_tables, ignore_classes, [r for r in (1, 2, 4, 8, 16) if r <= radius])
    seg_tables, seg_summary = {}, None
    if seg is not None:
        seg = seg.cpu()
        seg_tables = {name: seg[i] for i, name in enumerate(names)}
        seg_summary = summarise_segments(seg_tables, ignore_classes)
    cons_tables, cons_summary = {}, None
    if consistency:
        cons = cons.cpu()
        cons_tables = {"agree": cons.agree, "flips": cons.flips, "per_view": cons.per_view}
        cons_summary = summarise_consistency(cons_tables, ignore_classes)
    conf_tables, rel_tables = {}, {}
    if joint:
        side = num_classes + 1
        matrices = table[:len(names) * side * side].view(len(names), side, side)
        conf_tables = {name: matrices[i] for i, name in enumerate(names)}
        if bins > 0:
            rel = table[len(names) * side * side:].view(len(layers[0]), num_classes, bins, 2)
            rel_tables = {name: rel[i] for i, name in enumerate(layers[0])}
        table = counts_from_confusion(matrices)
    counts = {name: table[i] for i, name in enumerate(names)}
    per_class, mean, score = summarise_validation(counts, ignore_classes)
    losses = {k: stat_mean([row[i] for row in loss_rows]) for i, k in enumerate(keys)}
    return SimpleNamespace(losses=losses, counts=counts, per_class=per_class, mean=mean, checkpoint_score=score,
                           confusion=conf_tables, reliability=rel_tables, consistency=cons_tables, consistency_summary=cons_summary,
                           boundary=bound_tables, boundary_summary=bound_summary, segments=seg_tables, segment_summary=seg_summary)


def despeckle(labels, min_size, num_classes=19, fill=255, connectivity=8):
    """A copy of a TRAIN-ID label map (int64 or uint8 [B,H,W], 255 = no label) without its specks: every pixel of a connected
    segment (one class, `connectivity` 4 or 8) of fewer than `min_size` pixels holds `fill`; ops.segment_filter on the device.  Meant
    for the `teacher_labels` of a target step and for the maps of infer_label_maps / infer_label_maps_ms BEFORE a look-up table: a
    map that went through a LUT holds dataset ids, which are no classes in [0, num_classes) -- it must not be passed (its ids above
    num_classes would be left alone as "no class" and the others taken for the wrong classes' segments)."""
    from dasac_hip import ops
    return ops.segment_filter(labels, min_size, num_classes, fill, connectivity)


# --------------------------------------------------------------------------------------------------
# epoch summaries (base_trainer.py:75-218,272-278): the panel strip of the fixed batches, rendered on the device
# --------------------------------------------------------------------------------------------------
def visualise_results(net, batch, step="source", group_size=None, im_size=(256, 256), num_groups=None, palette=None, cmap=None,
                      mean=None, std=None):
    """`BaseTrainer.visualise_results` -> `step(..., train=False, visualise=True)` (base_trainer.py:272-278, train.py:140-141,
    235-236) for one fixed batch: eval mode under no_grad (the previous mode is restored), neither the teacher nor the class prior
    is updated (the contract of `validation`).

      step="source": batch (image, gt) -> `net(image, gt)` -> panels image, ground truth, prediction, confidence;
      step="target": batch (frames1, frames_gt, frames2, affine, affine_inv) as loaded, [N,T,...] each, through `prep_batch`
                     (`num_groups` defaults to loaded groups x world) -> `net(f1, gt, f2, affine, affine_inv, use_teacher=True,
                     update_teacher=False, T=group_size)` -> all thirteen panels, frames2 as `image2`.

    The panels are rendered by ONE kernel launch where the tensors are (visualise.render); the u8 rows -- not `net_outs` -- are
    gathered over the ranks, rank-major (visualise.gather_rows: host tensors under gloo), and stacked into the grid
    (visualise.to_grid).  Returns a namespace: grid u8 [3, rows, cols] on the HOST with every rank's rows (on every rank),
    names = the panel names in strip order, running_conf = the class prior as the reference logs it (list of C floats, None for
    the source step).  Writing stays the caller's: `writer.add_image(tag, grid, epoch, dataformats="CHW")` and
    `writer.add_scalar("running_conf/%02d" % i, conf, epoch)`."""
    from types import SimpleNamespace
    import visualise as V
    assert step in ("source", "target"), step
    core = _unwrap(net)
    device = next(core.parameters()).device
    _, world = _dist_state(None, None)
    kw = dict(im_size=im_size, palette=palette, cmap=cmap, mean=V.MEAN if mean is None else mean, std=V.STD if std is None else std,
              want_u8=True)
    with eval_mode(core), torch.no_grad():
        inputs, step_kw = _step_inputs(batch, step, group_size, num_groups, device, world)
        if inputs[1].device == batch[1].device:
            inputs[1] = inputs[1].clone()           # the forward pass rewrites -1 to 255 in place: not in the caller's batch
        _, outs = net(*inputs, **step_kw)
        image, gt, image2 = (inputs + [None])[:3]   # the source step has no second image
        gt = gt.view(-1, *gt.shape[-2:])
        names = V.panel_names(outs, image2)
        _, rows = V.render(image, gt, outs, image2=image2, **kw)
    rows, confs = V.gather_rows(rows, outs.get("running_conf"))
    return SimpleNamespace(grid=V.to_grid(rows.cpu()), names=names, running_conf=confs)
