"""Minimal training driver reproducing the reference's step order on one rank
(/root/reference/train.py:119-155 source step, :211-250 target step, :266-298 loop body,
/root/reference/base_trainer.py:47-73 optimiser factory).  Works on the bare module or on a
DistributedDataParallel wrapper (backend "nccl" == RCCL on ROCm)."""
import torch


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
    core = net.module if hasattr(net, "module") else net
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
    core = net.module if hasattr(net, "module") else net
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
    was = core.training
    core.eval()
    with torch.no_grad():
        ys = torch.cat([core(images[i:i + 1])[1].argmax(1) for i in range(images.shape[0])], 0)
    core.train(was)
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
    was = core.training
    core.eval()
    with torch.no_grad():
        std = float(core(image)[0].std())
        f = target_std / max(std, 1e-12)
        for m in _classifier_layers(core):
            m.weight.mul_(f)
            if m.bias is not None:
                m.bias.mul_(f)
    core.train(was)
    return f


# --------------------------------------------------------------------------------------------------
# checkpoints and validation
# --------------------------------------------------------------------------------------------------
def save_checkpoint(path, net, optim, score, epoch):
    """File layout of the reference's utils/checkpoints.py:62-74: {"model": state dict with the DDP
    "module." prefix, "opt": optimiser state, "score", "epoch"}."""
    core = net.module if hasattr(net, "module") else net
    model = {"module." + k: v for k, v in core.state_dict().items()}
    torch.save({"model": model, "opt": optim.state_dict() if optim is not None else None, "score": score, "epoch": epoch}, path)


def load_checkpoint(path, net, optim=None, map_location="cpu"):
    """utils/checkpoints.py:49-60: strict=False, so a baseline snapshot (backbone only) loads into SAC and
    leaves the teacher / class prior to the first `_momentum_update`.  Accepts keys with or without "module."."""
    blob = torch.load(path, map_location=map_location)
    core = net.module if hasattr(net, "module") else net
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
    core = net.module if hasattr(net, "module") else net
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


def infer_label_maps_ms(net, image, scales=(0.5, 0.75, 1.0), flip=True, mode="mean", lut=None, teacher=False, want_conf=False,
                        want_probs=False):
    """infer_label_maps with test-time augmentation: the image at every scale of `scales`, plain and (with `flip`) mirrored, the
    class probabilities of all of them fused by mean or max (`mode`) at the image's own size.  Per scale s the backbone sees
    scaled_size(H, W, s) pixels: ONE ops.image_pyramid launch makes the scaled (and mirrored) input -- none for s == 1.0 without
    flip, the image itself is passed -- and ONE `_logits` call runs it, at batch 2B when flipping; then ONE ops.infer_fuse launch
    over all the halves (the mirrored half is a batch slice of the same logits tensor) writes the uint8 label map.  No
    upsampled, flipped, softmaxed or summed [B,C,H,W] tensor exists; torch only allocates.  At most 8 sources (scales x
    orientations).  Returns (labels u8 [B,H,W], conf f32 [B,H,W] or None, probs f32 [B,C,H,W] or None): conf is the winning fused
    probability, probs all of them (infer_val.py's D_SAVE_RAW).  `lut`, `teacher` as infer_label_maps."""
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
        return ops.infer_fuse(sources, flips, (H, W), mode, lut, want_conf, want_probs)


def validation_iou(net, batches, num_classes=19, scales=None, flip=False, confusion=False, boundary_radius=0):
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
    {"prediction": table}).  0 changes nothing."""
    import torch.distributed as dist
    from dasac_hip import ops
    core = net.module if hasattr(net, "module") else net
    was = core.training
    core.eval()
    counts, boundary, radius = None, None, int(boundary_radius)
    multi_scale = scales is not None or flip
    with torch.no_grad():
        for image, gt in batches:
            if multi_scale:
                maps, _, _ = infer_label_maps_ms(net, image, (1.0,) if scales is None else scales, flip)
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
    core.train(was)
    if (multi_scale or confusion) and counts is not None:
        counts = counts[0]
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(counts)
        if boundary is not None:
            dist.all_reduce(boundary)
    matrix = counts.cpu() if confusion else None
    iou, _, _ = summarise_iou(counts_from_confusion(matrix) if confusion else counts)
    result = (float(iou.mean()), iou, matrix) if confusion else (float(iou.mean()), iou)
    return result + (boundary[0].cpu(),) if radius > 0 and boundary is not None else result


def summarise_iou(counts):
    """`Jaccard.summarise` (utils/metrics.py:40-53) on int64 counts [3, C] = (tp, fp, fn): per-class
    (jaccard, precision, recall) = tp / max(1e-3, .) in float32 like the reference (a class that never occurs scores 0)."""
    tp, fp, fn = (counts[i].to(torch.float32).cpu() for i in range(3))
    floor = torch.tensor(1e-3)
    return tp / torch.maximum(floor, fn + fp + tp), tp / torch.maximum(floor, tp + fp), tp / torch.maximum(floor, tp + fn)


def counts_from_confusion(matrix):
    """(tp, fp, fn) of a confusion matrix int64 [C+1,C+1] (row = ground truth, column = prediction, index C = no class; leading
    layer dimensions are kept): tp[c] = M[c][c], fp[c] = sum_r M[r][c] - M[c][c], fn[c] = sum_k M[c][k] - M[c][c] for c < C -- int64
    [..., 3, C] on the host, the integers ops.mask_counts counts (integer bookkeeping on a small host table)."""
    import numpy as np
    M = matrix.detach().cpu().numpy()
    C = M.shape[-1] - 1
    tp = np.diagonal(M, axis1=-2, axis2=-1)[..., :C]
    return torch.from_numpy(np.stack([tp, M[..., :, :C].sum(-2) - tp, M[..., :C, :].sum(-1) - tp], -2).astype(np.int64))


def _share(num, den):
    """num / den in float64 with 0 where den is 0."""
    num, den = num.to(torch.float64), den.to(torch.float64)
    return torch.where(den > 0, num / den.clamp_min(1.0), torch.zeros_like(num))


def summarise_confusion(matrix, ignore_classes=(), top=10):
    """Reading of one confusion matrix int64 [C+1,C+1] (host or device; the result is on the host).  Returns a namespace:
      by_gt, by_pred   the matrix divided by its ground-truth row sums / prediction column sums, float64; a zero row (column) stays 0;
      pixel_accuracy   correct pixels over the pixels whose ground truth is a class (a prediction of "no class" is wrong);
      fw_iou           sum_c freq_c * IoU_c with freq_c the class's share of those pixels and IoU_c = tp / (tp + fp + fn);
      top              the `top` largest off-diagonal entries [(gt, pred, pixels, share of the gt row)], largest first, ties by
                       (gt, pred); index C stands for "no class".
    Classes in `ignore_classes` leave the accuracy, the frequencies of fw_iou and, as row or column, the top list; every class's
    IoU is still computed on the whole matrix, as the class-subset means of `validation` are."""
    from types import SimpleNamespace
    M = matrix.detach().cpu().to(torch.int64)
    C = M.shape[0] - 1
    rows, cols = M.sum(1), M.sum(0)
    by_gt, by_pred = _share(M, rows[:, None].expand_as(M)), _share(M, cols[None, :].expand_as(M))
    ignore = set(int(i) for i in ignore_classes)
    keep = torch.tensor([c for c in range(C) if c not in ignore], dtype=torch.int64)
    tp, fp, fn = counts_from_confusion(M)
    labelled = rows[keep].sum()
    accuracy = float(_share(tp[keep].sum(), labelled))
    fw_iou = float((_share(rows[keep], labelled.expand(len(keep))) * _share(tp, tp + fp + fn)[keep]).sum())
    entries = [(int(M[r, c]), r, c) for r in range(C + 1) for c in range(C + 1)
               if r != c and r not in ignore and c not in ignore and int(M[r, c]) > 0]
    entries.sort(key=lambda t: (-t[0], t[1], t[2]))
    worst = [(r, c, n, float(by_gt[r, c])) for n, r, c in entries[:top]]
    return SimpleNamespace(by_gt=by_gt, by_pred=by_pred, pixel_accuracy=accuracy, fw_iou=fw_iou, top=worst)


def pseudo_label_audit(labels_matrix, teacher_matrix):
    """What the pseudo-label thresholds do per class, from the confusion matrices of `teacher_labels` (the thresholded label map,
    255 = rejected = column C) and `teacher_refined` (the same teacher before thresholding).  float64 [C] each, 0 where a class has
    no pixel:
      coverage           share of the class's ground-truth pixels that received any label: 1 - M[c][C] / sum_k M[c][k];
      precision          of the pixels labelled c, the share whose ground truth is c: M[c][c] / sum_r M[r][c];
      teacher_recall     M_t[c][c] / sum_k M_t[c][k] of the unthresholded teacher;
      teacher_precision  M_t[c][c] / sum_r M_t[r][c]."""
    from types import SimpleNamespace
    Ml, Mt = labels_matrix.detach().cpu().to(torch.int64), teacher_matrix.detach().cpu().to(torch.int64)
    C = Ml.shape[0] - 1
    rows = Ml[:C].sum(1)
    return SimpleNamespace(coverage=_share(rows - Ml[:C, C], rows), precision=_share(torch.diagonal(Ml)[:C], Ml[:, :C].sum(0)),
                           teacher_recall=_share(torch.diagonal(Mt)[:C], Mt[:C].sum(1)),
                           teacher_precision=_share(torch.diagonal(Mt)[:C], Mt[:, :C].sum(0)))


def summarise_reliability(table):
    """Reading of one reliability table int64 [C,n_bins,2] (arg-max class, confidence bin, miss / hit).  Returns a namespace with,
    per class, pixels int64 [C,n_bins], accuracy float64 [C,n_bins] (hits / pixels, 0 for an empty bin) and ece float64 [C]; and over
    all classes overall_pixels [n_bins], overall_accuracy [n_bins], overall_ece (float).  The expected calibration error is
    sum_b pixels_b / pixels * |accuracy_b - (b + 0.5) / n_bins|: it takes the bin MIDPOINT for the bin's confidence, because the table
    keeps no sum of confidences -- an approximation, off by up to half a bin width (0.5 / n_bins) from the usual definition."""
    from types import SimpleNamespace
    R = table.detach().cpu().to(torch.int64)
    n_bins = R.shape[1]
    mid = (torch.arange(n_bins, dtype=torch.float64) + 0.5) / n_bins

    def read(hit, pixels):
        acc = _share(hit, pixels)
        total = pixels.sum(-1, keepdim=True)
        return acc, (_share(pixels, total.expand_as(pixels)) * (acc - mid).abs()).sum(-1)
    pixels = R.sum(-1)
    acc, ece = read(R[..., 1], pixels)
    all_acc, all_ece = read(R[..., 1].sum(0), pixels.sum(0))
    return SimpleNamespace(pixels=pixels, accuracy=acc, ece=ece, overall_pixels=pixels.sum(0), overall_accuracy=all_acc,
                           overall_ece=float(all_ece))


def format_confusion(matrix, names):
    """Fixed-width text table of a confusion matrix int64 [C+1,C+1] for the log: one row per ground-truth class (`names`, C of them,
    then "none"), one column per prediction, pixel counts."""
    M = matrix.detach().cpu().to(torch.int64)
    names = [str(n) for n in names] + ["none"]
    assert len(names) == M.shape[0] == M.shape[1], (len(names), tuple(M.shape))
    width = max(6, len(str(int(M.max()))))
    head = max(len("gt \\ pred"), max(len(n) for n in names))
    lines = [" ".join(["gt \\ pred".ljust(head)] + [n[:width].rjust(width) for n in names])]
    for n, row in zip(names, M.tolist()):
        lines.append(" ".join([n.ljust(head)] + [str(v).rjust(width) for v in row]))
    return "\n".join(lines)


def summarise_boundary(tables, ignore_classes=(), radii=(1, 2, 4, 8)):
    """Reading of boundary tables (`validation(..., boundary_radius=R).boundary`: {layer: int64 [R+1,5,C]}, host or device; include/
    dasac_hip.h: dasac_boundary_counts).  Slot s < R of a table holds the pixels at Chebyshev distance s + 1 from a class contour, slot
    R everything further; the rows are tp, fp, fn (by the pixel's distance in the ground truth), pred (by its distance in the predicted
    map) and both.  Returns {layer: {r: dict}} for every r of `radii` (a radius above R is a ValueError), each dict with
      band_iou, band_miou            per-class IoU float32 [C] of the pixels within r of a ground-truth contour (the trimap band:
                                     slots < r of tp, fp, fn), and its mean over the classes not in `ignore_classes`;
      interior_iou, interior_miou    the same of all other pixels (slots >= r);
      boundary_iou, boundary_miou    Boundary IoU (Cheng et al., 2021): I / (G + P - I) with G = sum (tp + fn), P = sum pred, I = sum both
                                     over the slots < r -- the band inside the ground-truth mask against the band inside the predicted one;
      error_share                    of all fp + fn of the classes not ignored, the share inside the band (0 without any error);
      pixel_share                    of the pixels whose ground truth is such a class, the share inside the band.
    Ratios follow summarise_iou: float32, numerator / max(1e-3, denominator), so a class without a pixel scores 0; means are
    class_subset_mean; the two shares are python floats."""
    import numpy as np
    radii = [int(r) for r in radii]
    ignore = set(int(i) for i in ignore_classes)
    floor = torch.tensor(1e-3)
    out = {}
    for layer, table in tables.items():
        T = table.detach().cpu().numpy().astype(np.int64)             # small host tables: integer bookkeeping in numpy
        R, C = T.shape[0] - 1, T.shape[2]
        if any(r < 1 or r > R for r in radii):
            raise ValueError("summarise_boundary: radii {} for a table of radius {} (1..{} can be read from it)".format(radii, R, R))
        keep = [c for c in range(C) if c not in ignore]
        total = T.sum(0)
        out[layer] = {}
        for r in radii:
            band = T[:r].sum(0)
            inner = total - band
            G, P, I = (torch.from_numpy(v).to(torch.float32) for v in (band[0] + band[2], band[3], band[4]))
            rows = dict(band_iou=summarise_iou([torch.from_numpy(v) for v in band[:3]])[0],
                        interior_iou=summarise_iou([torch.from_numpy(v) for v in inner[:3]])[0],
                        boundary_iou=I / torch.maximum(floor, G + P - I))
            entry = {}
            for key, values in rows.items():
                entry[key] = values
                entry[key.replace("_iou", "_miou")] = class_subset_mean(values, ignore_classes)
            errors, pixels = int((total[1] + total[2])[keep].sum()), int((total[0] + total[2])[keep].sum())
            entry["error_share"] = int((band[1] + band[2])[keep].sum()) / errors if errors else 0.0
            entry["pixel_share"] = int((band[0] + band[2])[keep].sum()) / pixels if pixels else 0.0
            out[layer][r] = entry
    return out


def format_boundary(summary, names):
    """Fixed-width text of a `summarise_boundary` result for the log: per layer one line per radius with the three means and the
    two shares, then one row per class (`names`, C of them) with band / interior / Boundary IoU at every radius."""
    names = [str(n) for n in names]
    head = max(len("class"), max(len(n) for n in names))
    lines = []
    for layer, by_radius in summary.items():
        radii = sorted(by_radius)
        lines.append("{}: boundary bands".format(layer))
        for r in radii:
            e = by_radius[r]
            assert len(names) == len(e["band_iou"]), (len(names), len(e["band_iou"]))
            lines.append("  r={:<2d} band mIoU {:.4f}  interior mIoU {:.4f}  boundary mIoU {:.4f}  errors in band {:.4f}  pixels in band {:.4f}".format(
                r, e["band_miou"], e["interior_miou"], e["boundary_miou"], e["error_share"], e["pixel_share"]))
        lines.append(" ".join(["class".ljust(head)] + ["band@{0} intr@{0} bIoU@{0}".format(r).rjust(23) for r in radii]))
        for c, n in enumerate(names):
            lines.append(" ".join([n.ljust(head)] + ["{:.4f}  {:.4f}  {:.4f}".format(
                float(by_radius[r]["band_iou"][c]), float(by_radius[r]["interior_iou"][c]), float(by_radius[r]["boundary_iou"][c])).rjust(23)
                for r in radii]))
    return "\n".join(lines)


def summarise_consistency(tables, ignore_classes=(), top=10):
    """Reading of the view-consistency tables (`validation(..., consistency=True).consistency`, or `SAC.consistency_tables()`: a
    dict or anything with agree / flips / per_view, host or device; the result is plain host numbers).  Per pixel the kernel counted
    k, the teacher views that cover it, the consensus class c* (arg-max of the summed views) and m, the covered views whose own
    arg-max is c*: agree[c*][k][m], and agree[C][0][0] where no view reaches.  Every share below counts the pixels with k >= 2
    only -- a pixel seen by one view cannot disagree.  Returns a dict:
      classes               one dict per class c: pixels (k >= 2), agreement = sum m / sum k, unanimous = share with m == k, by_k =
                            [T+1] shares of those pixels seen by exactly k views (entries 0 and 1 are 0); all 0 without such pixels;
      agreement             sum_c pixels_c * agreement_c / sum_c pixels_c over the classes not in `ignore_classes`: pixel-weighted;
      class_mean_agreement  the plain mean of agreement_c over the classes not ignored that have any k >= 2 pixel;
      classes_present       how many those are;
      uncovered_share       agree[C][0][0] over all pixels;
      flips                 the `top` largest off-diagonal entries of flips + flips^T (a pair of covered views whose arg-maxes are a
                            and b, in either order): dicts with a < b, pairs, share_a and share_b = pairs over all pairs that involve
                            a (b), the agreeing ones on the diagonal included; largest first, ties by (a, b); ignored classes left out;
      views                 one dict per view slot t: coverage = covered pixels / all pixels, agreement = covered pixels whose
                            arg-max is c* / covered pixels.
    `agreement` is a label-free score of a checkpoint, with one caveat that no table can remove: a COLLAPSED model that predicts one
    class everywhere agrees with itself perfectly and scores 1.0.  `classes_present` stands next to the score for that reason --
    read them together (and `flips`, which is empty in that case)."""
    import numpy as np
    get = (lambda k: tables[k]) if isinstance(tables, dict) else (lambda k: getattr(tables, k))
    A, F, V = (get(k).detach().cpu().to(torch.int64).numpy() for k in ("agree", "flips", "per_view"))   # small host tables: numpy
    C, T = A.shape[0] - 1, A.shape[1] - 1
    ks = np.arange(T + 1, dtype=np.int64)
    multi = A[:C, 2:]                                             # [C, T-1, T+1]: k >= 2
    by_k_pixels = np.concatenate([np.zeros((C, min(2, T + 1)), np.int64), multi.sum(2)], 1)
    pixels = multi.sum((1, 2))
    sum_m, sum_k = (multi * ks[None, None, :]).sum((1, 2)), (multi.sum(2) * ks[None, 2:]).sum(1)
    unanimous = sum((A[:C, k, k] for k in range(2, T + 1)), np.zeros(C, np.int64))

    def share(num, den):
        return np.where(den > 0, num / np.maximum(den, 1), 0.0)
    agreement, una, by_k = share(sum_m, sum_k), share(unanimous, pixels), share(by_k_pixels, pixels[:, None])
    classes = [dict(pixels=int(pixels[c]), agreement=float(agreement[c]), unanimous=float(una[c]), by_k=by_k[c].tolist())
               for c in range(C)]
    ignore = set(int(i) for i in ignore_classes)
    kept = [c for c in range(C) if c not in ignore and int(pixels[c]) > 0]
    kept_pixels = sum(int(pixels[c]) for c in kept)
    total = int(A.sum())
    S = F + F.T - np.diag(np.diagonal(F))
    involved = S.sum(1)
    entries = [(int(S[a, b]), a, b) for a in range(C) for b in range(a + 1, C)
               if a not in ignore and b not in ignore and int(S[a, b]) > 0]
    entries.sort(key=lambda t: (-t[0], t[1], t[2]))
    flips = [dict(a=a, b=b, pairs=n, share_a=n / int(involved[a]), share_b=n / int(involved[b])) for n, a, b in entries[:top]]
    views = [dict(coverage=int(V[t, 0]) / total if total else 0.0, agreement=int(V[t, 1]) / int(V[t, 0]) if int(V[t, 0]) else 0.0)
             for t in range(T)]
    return dict(classes=classes,
                agreement=sum(int(pixels[c]) * float(agreement[c]) for c in kept) / kept_pixels if kept_pixels else 0.0,
                class_mean_agreement=sum(float(agreement[c]) for c in kept) / len(kept) if kept else 0.0,
                classes_present=len(kept), uncovered_share=int(A[C, 0, 0]) / total if total else 0.0, flips=flips, views=views)


def format_consistency(summary, names):
    """Fixed-width text table of a `summarise_consistency` result for the log: the scores, one row per class (`names`, C of them),
    the most frequent flips and one row per view slot."""
    names = [str(n) for n in names]
    assert len(names) == len(summary["classes"]), (len(names), len(summary["classes"]))
    head = max(len("class"), max(len(n) for n in names))
    n_k = len(summary["classes"][0]["by_k"]) if names else 0
    lines = ["view agreement {:.4f} (class mean {:.4f}, {} of {} classes present), uncovered {:.4f}".format(
        summary["agreement"], summary["class_mean_agreement"], summary["classes_present"], len(names), summary["uncovered_share"])]
    lines.append(" ".join(["class".ljust(head), "pixels".rjust(12), "agree".rjust(7), "unanim".rjust(7)] +
                          ["k={}".format(k).rjust(6) for k in range(2, n_k)]))
    for n, row in zip(names, summary["classes"]):
        lines.append(" ".join([n.ljust(head), str(row["pixels"]).rjust(12), "{:.4f}".format(row["agreement"]).rjust(7),
                               "{:.4f}".format(row["unanimous"]).rjust(7)] + ["{:.3f}".format(v).rjust(6) for v in row["by_k"][2:]]))
    if summary["flips"]:
        lines.append("flips: " + ", ".join("{} <-> {} {} ({:.3f} / {:.3f})".format(names[f["a"]], names[f["b"]], f["pairs"], f["share_a"],
                                                                               f["share_b"]) for f in summary["flips"]))
    lines.append("views: " + ", ".join("{}: covers {:.4f}, agrees {:.4f}".format(t, v["coverage"], v["agreement"])
                                       for t, v in enumerate(summary["views"])))
    return "\n".join(lines)


def gradient_report(net, optim, table=None, top=10):
    """Reading of a gradient health table (`optim.tensor_stats` by default, or e.g. `optim.measure_tensor_stats()`; fp64
    [n_params, 8], dasac_hip.optim.TENSOR_STATS_COLUMNS, rows in the flattened `param_groups` order).  THE ONE PLACE that copies
    the table to the host -- a synchronisation: call it when logging, not every step.  Names are those of
    `net.named_parameters()` (through `.module` if wrapped), lr is each group's.  Returns a plain dict:
      tensors     one dict per parameter, in table order: name, group, numel, grad_norm, share (of the global squared gradient
                  norm), g_maxabs, zero_share (g_zeros / numel), weight_norm, update_ratio (lr * ||g|| / ||w||, 0 where ||w|| is 0),
                  state_norm, nonfinite (count) and first_nonfinite (index tuple in the parameter's shape, or None);
      groups      the same aggregated per parameter group: group, lr, tensors, numel, grad_norm, share, g_maxabs, zero_share,
                  weight_norm, update_ratio, state_norm, nonfinite;
      grad_norm   the global L2 norm over the finite gradient entries;
      nonfinite   the names of the tensors with non-finite gradient entries;
      top         the names of the `top` tensors by share, largest first (ties by table order).
    A parameter without a pending gradient has a row of zeros: it is listed with grad_norm 0 and share 0."""
    import math
    import numpy as np
    core = net.module if hasattr(net, "module") else net
    names = {p: name for name, p in core.named_parameters()}
    T = (optim.tensor_stats if table is None else table).detach().cpu().to(torch.float64).numpy()
    params = [(gi, p) for gi, group in enumerate(optim.param_groups) for p in group["params"]]
    assert T.shape == (len(params), 8), (T.shape, len(params))
    total_sq = float(T[:, 0].sum())
    share = lambda sq: sq / total_sq if total_sq > 0 else 0.0
    ratio = lambda lr, g, w: lr * g / w if w > 0 else 0.0
    tensors = []
    for i, ((gi, p), row) in enumerate(zip(params, T.tolist())):
        g_norm, w_norm, lr = math.sqrt(row[0]), math.sqrt(row[5]), float(optim.param_groups[gi]["lr"])
        first = tuple(int(v) for v in np.unravel_index(int(row[3]) - 1, tuple(p.shape))) if row[3] > 0 else None
        tensors.append(dict(name=names.get(p, "param{}".format(i)), group=gi, numel=p.numel(), grad_norm=g_norm, share=share(row[0]),
                            g_maxabs=row[1], zero_share=row[4] / max(p.numel(), 1), weight_norm=w_norm,
                            update_ratio=ratio(lr, g_norm, w_norm), state_norm=math.sqrt(row[7]), nonfinite=int(row[2]),
                            first_nonfinite=first))
    groups = []
    for gi, group in enumerate(optim.param_groups):
        rows = T[[i for i, (g, _) in enumerate(params) if g == gi]].reshape(-1, 8)
        numel = sum(p.numel() for p in group["params"])
        g_norm, w_norm = math.sqrt(float(rows[:, 0].sum())), math.sqrt(float(rows[:, 5].sum()))
        groups.append(dict(group=gi, lr=float(group["lr"]), tensors=len(group["params"]), numel=numel, grad_norm=g_norm,
                           share=share(float(rows[:, 0].sum())), g_maxabs=float(rows[:, 1].max()) if len(rows) else 0.0,
                           zero_share=float(rows[:, 4].sum()) / max(numel, 1), weight_norm=w_norm,
                           update_ratio=ratio(float(group["lr"]), g_norm, w_norm), state_norm=math.sqrt(float(rows[:, 7].sum())),
                           nonfinite=int(rows[:, 2].sum())))
    order = sorted(range(len(tensors)), key=lambda i: (-tensors[i]["share"], i))
    return dict(tensors=tensors, groups=groups, grad_norm=math.sqrt(total_sq), nonfinite=[t["name"] for t in tensors if t["nonfinite"]],
                top=[tensors[i]["name"] for i in order[:top]])


def skipped_step_report(net, optim, top=10):
    """`gradient_report` over `optim.last_skipped_stats` -- the table of the last step that `skip_nonfinite` skipped -- plus
    `captured_at`: `optim.skipped_steps` as it stood right after that step (0: no step has been skipped, the table is zeros)."""
    table, at = optim.last_skipped_stats
    report = gradient_report(net, optim, table=table, top=top)
    report["captured_at"] = int(at)
    return report


def format_gradient_report(report, top=10):
    """Fixed-width text table of a `gradient_report` for the log: the `top` tensors by share of the squared gradient norm, then
    every tensor with non-finite entries that is not among them, then one line per group and the global norm."""
    by_share = sorted(range(len(report["tensors"])), key=lambda i: (-report["tensors"][i]["share"], i))[:top]
    shown = by_share + [i for i, t in enumerate(report["tensors"]) if t["nonfinite"] and i not in by_share]
    rows = [report["tensors"][i] for i in shown]
    labels = ["group {} (lr {:.3g}, {} tensors)".format(g["group"], g["lr"], g["tensors"]) for g in report["groups"]]
    head = max([len("tensor")] + [len(t["name"]) for t in rows] + [len(l) for l in labels])
    cols = ["group", "numel", "|g|", "share", "max|g|", "zeros", "|w|", "lr|g|/|w|", "|state|", "nonfinite", "first"]
    width = [5, 9, 10, 7, 10, 7, 10, 10, 10, 9, 5]

    def cells(t):
        return [str(t["group"]), str(t["numel"]), "{:.3e}".format(t["grad_norm"]), "{:.4f}".format(t["share"]), "{:.3e}".format(t["g_maxabs"]),
                "{:.4f}".format(t["zero_share"]), "{:.3e}".format(t["weight_norm"]), "{:.3e}".format(t["update_ratio"]),
                "{:.3e}".format(t["state_norm"]), str(t["nonfinite"])]
    lines = [" ".join(["tensor".ljust(head)] + [c.rjust(w) for c, w in zip(cols, width)])]
    for t in rows:
        first = "-" if t["first_nonfinite"] is None else str(t["first_nonfinite"])
        lines.append(" ".join([t["name"].ljust(head)] + [c.rjust(w) for c, w in zip(cells(t), width)] + [first]))
    for name, g in zip(labels, report["groups"]):
        lines.append(" ".join([name.ljust(head)] + [c.rjust(w) for c, w in zip(cells(g), width)] + ["-"]))
    lines.append("global gradient norm {:.6e}; tensors with non-finite entries: {}".format(
        report["grad_norm"], ", ".join(report["nonfinite"]) if report["nonfinite"] else "none"))
    if "captured_at" in report:
        lines.append("captured at skipped step {}".format(report["captured_at"]))
    return "\n".join(lines)


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
    core = net.module if hasattr(net, "module") else net
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


def _host_table(record):
    import numpy as np
    T = record.table
    T = T.detach().cpu().to(torch.float64).numpy() if isinstance(T, torch.Tensor) else np.asarray(T, dtype=np.float64)
    R = sum(e["C"] for e in record.layout)
    assert T.ndim == 3 and T.shape == (len(record.bounds) - 1, R, 6), (T.shape, len(record.bounds) - 1, R)
    return T


def activation_report(record, segment=0, top=10):
    """Reading of one segment of an activation table.  THE ONE PLACE that copies it to the host -- a synchronisation: call it when
    logging.  Returns a plain dict:
      layers   one dict per tensor in plan order: name, kind, shape (n, C, H, W with n the segment's samples), mean and std over
               the finite entries of all channels, maxabs, zero_share (zeros / elements), dead_channels (channels whose every
               entry is 0: a dead ReLU unit), nonfinite (count) and first_nonfinite ((n, c, y, x) in the tensor, or None);
      first_nonfinite_layer   the name of the first layer in plan order with non-finite entries, or None: where a fault began;
      top      the names of the `top` layers by maxabs, largest first (ties in plan order);
      net, segment, samples (first, one past the last)."""
    import math
    import numpy as np
    T = _host_table(record)[segment]
    lo, hi = record.bounds[segment], record.bounds[segment + 1]
    layers = []
    for e in record.layout:
        rows = T[e["row0"]:e["row0"] + e["C"]]
        per_channel = (hi - lo) * e["H"] * e["W"]
        total, finite = per_channel * e["C"], per_channel * e["C"] - float(rows[:, 3].sum())
        mean = float(rows[:, 0].sum()) / finite if finite > 0 else 0.0
        var = max(float(rows[:, 1].sum()) / finite - mean * mean, 0.0) if finite > 0 else 0.0
        firsts = rows[:, 4][rows[:, 4] > 0]
        first = tuple(int(v) for v in np.unravel_index(int(firsts.min()) - 1, (record.N, e["C"], e["H"], e["W"]))) if len(firsts) else None
        layers.append(dict(name=e["name"], kind=e["kind"], shape=(hi - lo, e["C"], e["H"], e["W"]), mean=mean, std=math.sqrt(var),
                           maxabs=float(rows[:, 2].max()), zero_share=float(rows[:, 5].sum()) / total,
                           dead_channels=int((rows[:, 5] == per_channel).sum()), nonfinite=int(rows[:, 3].sum()), first_nonfinite=first))
    bad = [l["name"] for l in layers if l["nonfinite"]]
    order = sorted(range(len(layers)), key=lambda i: (-layers[i]["maxabs"], i))
    return dict(layers=layers, first_nonfinite_layer=bad[0] if bad else None, top=[layers[i]["name"] for i in order[:top]],
                net=record.net, segment=segment, samples=(lo, hi))


def moment_gap(mu_a, var_a, mu_b, var_b):
    """The per-channel distance of two sets of moments that `domain_gap_report` and `class_gap_report` share (numpy float64,
    broadcasting): num = (mu_a - mu_b)^2 + (sigma_a - sigma_b)^2, den = (var_a + var_b) / 2, 0 where num == 0, else
    num / max(den, 1e-30)."""
    import numpy as np
    num = (mu_a - mu_b) ** 2 + (np.sqrt(var_a) - np.sqrt(var_b)) ** 2
    return np.where(num == 0, 0.0, num / np.maximum(0.5 * (var_a + var_b), 1e-30))


def domain_gap_report(a, b=None, top=10):
    """Per-layer covariate shift between two domains under the same weights: two records of the same net (segment 0 of each), or
    ONE record with two segments (segments 0 and 1: `forward_fused`'s [source; target] batch).  Copies the tables to the host.
    Per channel, with n elements per domain: mu = sum / n, var = max(sumsq / n - mu^2, 0), sigma = sqrt(var),
      num = (mu_a - mu_b)^2 + (sigma_a - sigma_b)^2,  den = (var_a + var_b) / 2,  gap_c = 0 if num == 0 else num / max(den, 1e-30).
    Returns a plain dict:
      layers   one dict per tensor in plan order: name, kind, gap (mean of gap_c over the channels that are not dead -- all
               zero -- in BOTH domains; 0 if none), gap_max and gap_max_channel, mean_shift (RMS over channels of mu_a - mu_b),
               dead_only_a, dead_only_b, dead_both (channel counts);
      top      the names of the `top` layers by gap, largest first (ties in plan order).
    Refuses records whose layouts differ."""
    import numpy as np
    if b is None:
        if len(a.bounds) < 3:
            raise ValueError("domain_gap_report: one record needs two segments (got bounds {})".format(a.bounds))
        b, sa, sb = a, 0, 1
    else:
        sa = sb = 0
    same = lambda e: (e["name"], e["kind"], e["C"], e["H"], e["W"], e["row0"])
    if [same(e) for e in a.layout] != [same(e) for e in b.layout]:
        raise ValueError("domain_gap_report: the two records have different layouts")
    Ta, Tb = _host_table(a)[sa], _host_table(b)[sb]
    layers = []
    for e in a.layout:
        rows = slice(e["row0"], e["row0"] + e["C"])
        na = float((a.bounds[sa + 1] - a.bounds[sa]) * e["H"] * e["W"])
        nb = float((b.bounds[sb + 1] - b.bounds[sb]) * e["H"] * e["W"])
        mu_a, mu_b = Ta[rows, 0] / na, Tb[rows, 0] / nb
        var_a, var_b = np.maximum(Ta[rows, 1] / na - mu_a ** 2, 0.0), np.maximum(Tb[rows, 1] / nb - mu_b ** 2, 0.0)
        gap_c = moment_gap(mu_a, var_a, mu_b, var_b)
        dead_a, dead_b = Ta[rows, 5] == na, Tb[rows, 5] == nb
        alive = ~(dead_a & dead_b)
        worst = int(np.argmax(gap_c))
        layers.append(dict(name=e["name"], kind=e["kind"], gap=float(gap_c[alive].mean()) if alive.any() else 0.0,
                           gap_max=float(gap_c[worst]), gap_max_channel=worst, mean_shift=float(np.sqrt(np.mean((mu_a - mu_b) ** 2))),
                           dead_only_a=int((dead_a & ~dead_b).sum()), dead_only_b=int((dead_b & ~dead_a).sum()),
                           dead_both=int((dead_a & dead_b).sum())))
    order = sorted(range(len(layers)), key=lambda i: (-layers[i]["gap"], i))
    return dict(layers=layers, top=[layers[i]["name"] for i in order[:top]], net=a.net)


def _fixed_width(head, cols, width, names, cells):
    lines = [" ".join(["layer".ljust(head)] + [c.rjust(w) for c, w in zip(cols, width)])]
    for name, row in zip(names, cells):
        lines.append(" ".join([name.ljust(head)] + [c.rjust(w) for c, w in zip(row, width)]))
    return lines


def format_activation_report(report, top=10):
    """Fixed-width text table of an `activation_report` for the log: the `top` layers by maxabs, then every layer with non-finite
    entries that is not among them (plan order), then one summary line."""
    L_ = report["layers"]
    by_max = sorted(range(len(L_)), key=lambda i: (-L_[i]["maxabs"], i))[:top]
    rows = [L_[i] for i in by_max + [i for i, l in enumerate(L_) if l["nonfinite"] and i not in by_max]]
    head = max([len("layer")] + [len(l["name"]) for l in rows])
    cols, width = ["kind", "shape", "mean", "std", "max|x|", "zeros", "dead", "nonfinite", "first"], [6, 18, 11, 10, 10, 7, 5, 9, 5]
    cells = [[l["kind"], "x".join(str(v) for v in l["shape"]), "{:.3e}".format(l["mean"]), "{:.3e}".format(l["std"]),
              "{:.3e}".format(l["maxabs"]), "{:.4f}".format(l["zero_share"]), str(l["dead_channels"]), str(l["nonfinite"]),
              "-" if l["first_nonfinite"] is None else str(l["first_nonfinite"])] for l in rows]
    lines = _fixed_width(head, cols, width, [l["name"] for l in rows], cells)
    lines.append("{} segment {} (samples {}..{}): {} layers; first layer with non-finite entries: {}".format(
        report["net"], report["segment"], report["samples"][0], report["samples"][1] - 1, len(L_), report["first_nonfinite_layer"] or "none"))
    return "\n".join(lines)


def format_domain_gap_report(report, top=10):
    """Fixed-width text table of a `domain_gap_report`: the `top` layers by gap, largest first, then one summary line."""
    L_ = report["layers"]
    rows = [L_[i] for i in sorted(range(len(L_)), key=lambda i: (-L_[i]["gap"], i))[:top]]
    head = max([len("layer")] + [len(l["name"]) for l in rows])
    cols, width = ["kind", "gap", "gap_max", "channel", "mean_shift", "dead_a", "dead_b", "dead_ab"], [6, 10, 10, 7, 10, 6, 6, 7]
    cells = [[l["kind"], "{:.3e}".format(l["gap"]), "{:.3e}".format(l["gap_max"]), str(l["gap_max_channel"]), "{:.3e}".format(l["mean_shift"]),
              str(l["dead_only_a"]), str(l["dead_only_b"]), str(l["dead_both"])] for l in rows]
    lines = _fixed_width(head, cols, width, [l["name"] for l in rows], cells)
    lines.append("{}: {} layers; largest gap: {}".format(report["net"], len(L_), rows[0]["name"] if rows else "none"))
    return "\n".join(lines)


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
    core = net.module if hasattr(net, "module") else net
    backbone, _ = _infer_backbone_and_lut(net, None, None, teacher)
    tag = "slow_net" if (teacher and hasattr(core, "backbone")) else "backbone"
    radius, num_classes = int(radius), int(num_classes)
    record, eng = into, None
    was = core.training
    core.eval()
    try:
        with torch.no_grad():
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
    finally:
        core.train(was)
    if record is None:
        raise ValueError("class_features: no batches")
    return record


def reduce_class_features(record):
    """Sums a record's table over the ranks of the process group, in place: one collective for `sums`, one for `counts` (both
    add).  gloo moves device tensors with no ordering against the stream that fills them (see prep_batch), so under gloo the HOST
    tensors are summed and the record then holds host tensors; RCCL sums on the device.  Without a process group (or with one
    rank) nothing happens.  Returns the record."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return record
    table = record.table.cpu() if dist.get_backend() == "gloo" else record.table
    dist.all_reduce(table.sums)
    dist.all_reduce(table.counts)
    record.table = table
    return record


def _class_moments(record):
    """(n [C], mu [C,Cf], var [C,Cf], dead [C,Cf]) in numpy float64 from a ClassFeatureRecord, a ClassFeatureTable or anything with
    `sums` / `counts` (torch tensors or arrays): the one host copy."""
    import numpy as np
    table = getattr(record, "table", record)
    host = lambda t, dt: t.detach().cpu().numpy().astype(dt) if isinstance(t, torch.Tensor) else np.asarray(t, dtype=dt)
    sums, counts = host(table.sums, np.float64), host(table.counts, np.int64)
    assert sums.ndim == 3 and sums.shape[2] == 2 and counts.shape == (sums.shape[0],), (sums.shape, counts.shape)
    n = np.maximum(counts, 1).astype(np.float64)[:, None]
    mu = sums[..., 0] / n
    var = np.maximum(sums[..., 1] / n - mu ** 2, 0.0)
    return counts, mu, var, sums[..., 1] == 0


def _row_distance(mu_a, var_a, dead_a, mu_b, var_b, dead_b):
    """D of two class rows: `moment_gap` averaged over the channels that are not dead (all zero) in both; 0 if there is none."""
    alive = ~(dead_a & dead_b)
    return float(moment_gap(mu_a, var_a, mu_b, var_b)[alive].mean()) if alive.any() else 0.0


def class_gap_report(a, b=None, ignore_classes=(), min_nodes=16, top=5):
    """Reads two class feature tables -- `a` (say, the source) against `b` (the target) -- or `a` alone.  Host-side float64; THE ONE
    PLACE that copies the tables to the host.  Per class c with n_c nodes: mu_c[f] = sum / n_c, var_c[f] = max(sumsq / n_c - mu^2,
    0).  D(row, row') is `domain_gap_report`'s per-channel formula (`moment_gap`) averaged over the channels not dead in both rows.
    A class counts in a table when it is not in `ignore_classes` and has at least `min_nodes` nodes there.  With `b`, per class c
    that counts in both:
      gap[c]      D(a_c, b_c): how far the class moved between the domains;
      nearest[c]  argmin over k != c (k counting in a) of D(b_c, a_k), with nearest_distance[c];
      margin[c]   nearest_distance[c] / gap[c]: below 1, b's class c lies nearer to ANOTHER class of a than to its own (inf when
                  gap is 0).
    Returns a plain dict: gap, nearest (-1: none), nearest_distance, margin (numpy [C]; NaN for the classes in `skipped`), matrix
    [C,C] = D(b_c, a_k) (NaN where c does not count in b or k not in a), counts_a, counts_b, skipped ({class: reason} -- "ignored",
    "absent" or "under min_nodes"), top (the `top` classes by margin, smallest first), layer, Cf.
    With b=None the same within `a`: matrix = D(a_c, a_k) with a zero diagonal, gap = 0, margin = inf, and top lists the classes by
    nearest_distance, smallest first -- class separability.  Refuses tables of different shapes or, for records, layers."""
    import numpy as np
    within = b is None
    if within:
        b = a
    na, mu_a, var_a, dead_a = _class_moments(a)
    nb, mu_b, var_b, dead_b = _class_moments(b)
    if mu_a.shape != mu_b.shape:
        raise ValueError("class_gap_report: tables of different shapes {} and {}".format(mu_a.shape, mu_b.shape))
    if getattr(a, "layer", None) != getattr(b, "layer", None):
        raise ValueError("class_gap_report: records of different layers {!r} and {!r}".format(getattr(a, "layer", None), getattr(b, "layer", None)))
    C, Cf = mu_a.shape
    ignored = set(int(c) for c in ignore_classes)
    in_a = [c not in ignored and na[c] >= max(int(min_nodes), 1) for c in range(C)]
    in_b = [c not in ignored and nb[c] >= max(int(min_nodes), 1) for c in range(C)]
    skipped = {}
    for c in range(C):
        if not (in_a[c] and in_b[c]):
            skipped[c] = "ignored" if c in ignored else ("absent" if min(na[c], nb[c]) == 0 else "under min_nodes")
    matrix = np.full((C, C), np.nan)
    for c in range(C):
        for k in range(C):
            if in_b[c] and in_a[k]:
                matrix[c, k] = 0.0 if (within and c == k) else _row_distance(mu_b[c], var_b[c], dead_b[c], mu_a[k], var_a[k], dead_a[k])
    gap, dist, margin = np.full(C, np.nan), np.full(C, np.nan), np.full(C, np.nan)
    nearest = np.full(C, -1, dtype=np.int64)
    for c in range(C):
        if c in skipped:
            continue
        gap[c] = matrix[c, c]
        others = [k for k in range(C) if k != c and in_a[k]]
        if others:
            nearest[c] = min(others, key=lambda k: (matrix[c, k], k))
            dist[c] = matrix[c, nearest[c]]
            margin[c] = dist[c] / gap[c] if gap[c] > 0 else (np.inf if dist[c] > 0 or within else np.nan)
    key = dist if within else margin
    order = sorted([c for c in range(C) if c not in skipped and nearest[c] >= 0], key=lambda c: (key[c], c))
    return dict(gap=gap, nearest=nearest, nearest_distance=dist, margin=margin, matrix=matrix, counts_a=na, counts_b=nb,
                skipped=skipped, top=order[:top], layer=getattr(a, "layer", None), Cf=Cf, within=within)


def format_class_gap_report(report, names=None):
    """Fixed-width text table of a `class_gap_report`: one line per class that counts, by margin (alone: by nearest distance),
    smallest first, then one summary line.  names: class names (default: the indices)."""
    C = len(report["gap"])
    name = lambda c: str(c) if c < 0 or names is None else str(names[c])
    key = report["nearest_distance"] if report["within"] else report["margin"]
    rows = sorted([c for c in range(C) if c not in report["skipped"]], key=lambda c: (key[c] != key[c], key[c], c))
    head = max([len("class")] + [len(name(c)) for c in rows])
    near = max([len("nearest")] + [len(name(int(report["nearest"][c]))) for c in rows])
    cols, width = ["n_a", "n_b", "gap", "nearest", "distance", "margin"], [9, 9, 10, near, 10, 10]
    lines = [" ".join(["class".ljust(head)] + [c.rjust(w) for c, w in zip(cols, width)])]
    for c in rows:
        k = int(report["nearest"][c])
        cells = [str(int(report["counts_a"][c])), str(int(report["counts_b"][c])), "{:.3e}".format(report["gap"][c]),
                 name(k) if k >= 0 else "-", "{:.3e}".format(report["nearest_distance"][c]), "{:.3e}".format(report["margin"][c])]
        lines.append(" ".join([name(c).ljust(head)] + [v.rjust(w) for v, w in zip(cells, width)]))
    below = [c for c in rows if report["margin"][c] < 1]
    lines.append("{}: {} channels, {} of {} classes compared, {} skipped; margin below 1: {}".format(
        report["layer"] or "table", report["Cf"], len(rows), C, len(report["skipped"]), ", ".join(name(c) for c in below) or "none"))
    return "\n".join(lines)


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
    import torch.distributed as dist
    from dasac_hip import ops
    core = net.module if hasattr(net, "module") else net
    was = core.training
    core.eval()
    table = torch.zeros((num_images, 256), dtype=torch.int64, device=next(core.parameters()).device)
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
    core.train(was)
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return table.cpu()
    # gloo moves device tensors with no ordering against the stream that fills them (see prep_batch): with it the HOST
    # tables are summed; RCCL sums on the device, stream-ordered, before the one D2H copy.
    if dist.get_backend() == "gloo":
        table = table.cpu()
    dist.all_reduce(table)
    return table.cpu()


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


def stat_mean(values):
    """`StatManager.update_stats` + `summarize_key` (utils/stat_manager.py:40-61) over one key's values: python-float sum
    divided by the count, and 0 when there is no value or the sum is exactly 0."""
    total = 0.0
    for v in values:
        total += v
    return total / len(values) if len(values) > 0 and abs(total) > 0. else 0


def class_subset_mean(values, ignore_classes=()):
    """train.py:370-371,447-460: float32 mean over the classes NOT listed in VAL.IGNORE_CLASS."""
    ignore = set(int(i) for i in ignore_classes)
    return torch.Tensor([float(v) for i, v in enumerate(values) if i not in ignore]).mean().item()


def summarise_validation(counts, ignore_classes=()):
    """counts {layer: int64 [3,C]} -> (per_class {layer: (jaccard, precision, recall)}, mean {layer: (mIoU, precision,
    recall)} over the kept classes, checkpoint_score = max over layers of mIoU, starting from 0.0: train.py:408,430-464)."""
    per_class, mean, score = {}, {}, 0.0
    for layer, table in counts.items():
        per_class[layer] = summarise_iou(table)
        mean[layer] = tuple(class_subset_mean(v, ignore_classes) for v in per_class[layer])
        score = max(mean[layer][0], score)
    return per_class, mean, score


def validation(net, loader, step="source", group_size=None, max_iter=None, ignore_classes=(), num_classes=19, num_groups=None,
               confusion=False, reliability_bins=0, consistency=False, consistency_cover=0.5, boundary_radius=0):
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
    over ranks (gloo: the HOST table, see compute_sample_weights; RCCL: on the device).  `max_iter`: see validation_batches.
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
    (format_boundary renders it); {} and None when off.  Reported only: every other field is the one of a run without it."""
    from types import SimpleNamespace
    import torch.distributed as dist
    from dasac_hip import ops
    assert step in ("source", "target"), step
    if consistency and step != "target":
        raise ValueError("validation: view consistency needs the teacher's aligned views, step='target' (got step={!r})".format(step))
    core = net.module if hasattr(net, "module") else net
    if consistency and not hasattr(core, "swap_consistency"):
        raise ValueError("validation: {} collects no view consistency".format(type(core).__name__))
    device = next(core.parameters()).device
    rank, world = _dist_state(None, None)
    was = core.training
    core.eval()
    joint, bins = bool(confusion) or int(reliability_bins) > 0, int(reliability_bins)
    layers, table, rows, keys, matrices, rel = None, None, [], None, None, None
    cons, cons_was = None, None
    radius, bound = int(boundary_radius), None
    if consistency:
        cons_was = core.swap_consistency((True, consistency_cover, None))
    try:
        with torch.no_grad():
            for batch in validation_batches(loader, max_iter):
                if step == "source":
                    image, gt = (t.to(device, non_blocking=True) for t in batch)
                    losses, outs = net(image, gt)
                else:
                    groups = num_groups if num_groups is not None else batch[0].shape[0] * world
                    f1, gt, f2, affine, affine_inv = (prep_batch(t, groups, group_size, device=device) for t in batch)
                    losses, outs = net(f1, gt, f2, affine, affine_inv, use_teacher=True, update_teacher=False, T=group_size)
                gt = gt.view(-1, *gt.shape[-2:])
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
                rows.append(torch.cat([losses[k].detach().mean().reshape(1) for k in keys]))
    finally:
        core.train(was)
        if consistency:
            cons = core.swap_consistency(cons_was)[2]
    if table is None:
        return SimpleNamespace(losses={}, counts={}, per_class={}, mean={}, checkpoint_score=0.0, confusion={}, reliability={},
                               consistency={}, consistency_summary=None, boundary={}, boundary_summary=None)
    if consistency and cons is None:        # a rank that owns no group (views sharded over ranks) still takes part in the sum
        cons = ops.consistency_tables(num_classes, group_size, device)
    names = layers[0] + layers[1]
    loss_rows = torch.stack(rows)
    multi = dist.is_available() and dist.is_initialized() and world > 1
    if multi:
        # gloo moves device tensors with no ordering against the stream that fills them (see prep_batch): the HOST tables are
        # summed; RCCL sums on the device, stream-ordered, before the one D2H copy.
        if dist.get_backend() == "gloo":
            table, loss_rows = table.cpu(), loss_rows.cpu()
        dist.all_reduce(table)
        if step == "target":
            dist.all_reduce(loss_rows)
            loss_rows = loss_rows / world
        if consistency:
            if dist.get_backend() == "gloo":
                cons = cons.cpu()
            dist.all_reduce(cons.buffer)
        if bound is not None:
            if dist.get_backend() == "gloo":
                bound = bound.cpu()
            dist.all_reduce(bound)
    table, loss_rows = table.cpu(), loss_rows.cpu().tolist()
    bound_tables, bound_summary = {}, None
    if bound is not None:
        bound = bound.cpu()
        bound_tables = {name: bound[i] for i, name in enumerate(names)}
        bound_summary = summarise_boundary(bound_tables, ignore_classes, [r for r in (1, 2, 4, 8, 16) if r <= radius])
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
                           boundary=bound_tables, boundary_summary=bound_summary)


# --------------------------------------------------------------------------------------------------
# epoch summaries (base_trainer.py:75-218,272-278): the panel strip of the fixed batches, rendered on the device
# --------------------------------------------------------------------------------------------------
from visualise import FixedBatches  # noqa: E402,F401  (`save_fixed_batch` / `has_fixed_batch`, base_trainer.py:200-218)


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
    core = net.module if hasattr(net, "module") else net
    device = next(core.parameters()).device
    _, world = _dist_state(None, None)
    kw = dict(im_size=im_size, palette=palette, cmap=cmap, mean=V.MEAN if mean is None else mean, std=V.STD if std is None else std,
              want_u8=True)
    was = core.training
    core.eval()
    try:
        with torch.no_grad():
            if step == "source":
                image, gt = (t.to(device, non_blocking=True) for t in batch[:2])
                if gt.device == batch[1].device:
                    gt = gt.clone()                 # the forward pass rewrites -1 to 255 in place: not in the caller's batch
                _, outs = net(image, gt)
                image2 = None
            else:
                groups = num_groups if num_groups is not None else batch[0].shape[0] * world
                image, gt, image2, affine, affine_inv = (prep_batch(t, groups, group_size, device=device) for t in batch)
                if gt.device == batch[1].device:
                    gt = gt.clone()
                _, outs = net(image, gt, image2, affine, affine_inv, use_teacher=True, update_teacher=False, T=group_size)
            gt = gt.view(-1, *gt.shape[-2:])
            names = V.panel_names(outs, image2)
            _, rows = V.render(image, gt, outs, image2=image2, **kw)
    finally:
        core.train(was)
    rows, confs = V.gather_rows(rows, outs.get("running_conf"))
    return SimpleNamespace(grid=V.to_grid(rows.cpu()), names=names, running_conf=confs)
