"""The trainer's epoch summary panels (base_trainer.py:75-198 `BaseTrainer._visualise`, helpers :220-270) rendered on the device.

The reference gathers every entry of `net_outs` over the ranks, copies it to the host and runs softmax, bilinear resizing,
arg-max, Pillow palettes and matplotlib colour maps there.  Here ONE kernel launch per batch (`ops.vis_panels`) renders the
panel strip where the tensors are, and what crosses PCIe and the ranks is the rendered rows, never `net_outs`:

    strip, rows = render(image, masks_gt, outs, image2=frames2, want_u8=True)     # float32 / u8 [B,3,h,P*w] on the device
    rows, confs = gather_rows(rows, outs.get("running_conf"))                     # rank-major, all ranks' rows
    grid = to_grid(rows)                                                          # u8 [3, rows, cols]: writer.add_image(..., "CHW")

Panels, in this order, each present when its input is (base_trainer.py:118-187):
    image | ground_truth | teacher_labels | prediction | confidence | image2 | teacher_conf |
    teacher_init, teacher_init_conf | teacher_aligned, teacher_aligned_conf | teacher_refined, teacher_refined_conf
Not reproduced: `denorm` mutating its argument in place, `downsize`'s `.squeeze()` breaking a batch of one, the min-entropy
colouring the reference computes and discards (`compute_entpy_rgb`, the first `_mask_rgb` result)."""
import numpy as np
import torch

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)          # datasets/dataloader_base.py:39-40
IM_SIZE = (256, 256)                                               # TB.IM_SIZE, core/config.py:173
GRID_PADDING, GRID_PAD_VALUE = 8, 0.9                              # base_trainer.py:269

# Cityscapes train-id colours (cityscapesScripts `labels`; the reference's tools/category.py through utils/palette.py)
CS_TRAIN_COLOURS = ((128, 64, 128), (244, 35, 232), (70, 70, 70), (102, 102, 156), (190, 153, 153), (153, 153, 153), (250, 170, 30),
                    (220, 220, 0), (107, 142, 35), (152, 251, 152), (70, 130, 180), (220, 20, 60), (255, 0, 0), (0, 0, 142), (0, 0, 70),
                    (0, 60, 100), (0, 80, 100), (0, 0, 230), (119, 11, 32))


def _cs_palette():
    pal = np.zeros((256, 3), np.uint8)
    pal[:len(CS_TRAIN_COLOURS)] = np.array(CS_TRAIN_COLOURS, np.uint8)
    pal.setflags(write=False)
    return pal


CS_PALETTE = _cs_palette()       # u8 [256,3]: indices 0..18 the train-id colours, every other index black


def palette_index(labels):
    """What `_apply_cmap` (base_trainer.py:228-248) makes of a label before the palette lookup: Pillow's
    `Image.fromarray(uint32).convert("P")` saturates to 0..255 -- -1 becomes 0, 300 becomes 255."""
    return np.clip(np.asarray(labels).astype(np.int64), 0, 255).astype(np.uint8)


def colormap(name="inferno", table=None):
    """float32 [256,3] table of a matplotlib colour map, what `cm.get_cmap(name)(v)[..., :3]` indexes with trunc(256 * v)
    (base_trainer.py:143,250-256).  Taken from matplotlib when it is importable (the reference needs it too); otherwise the
    caller passes the [256,3] table."""
    if table is None:
        try:
            import matplotlib
        except ImportError:
            raise RuntimeError("colormap({!r}): matplotlib is not importable; pass table=<[256,3] array> instead".format(name))
        table = matplotlib.colormaps[name](np.arange(256))[:, :3]
    table = np.ascontiguousarray(np.asarray(table, dtype=np.float32))
    if table.shape != (256, 3):
        raise ValueError("a colour map is a [256,3] table (got {})".format(table.shape))
    return table


PANELS = ("image", "ground_truth", "teacher_labels", "prediction", "confidence", "image2", "teacher_conf", "teacher_init",
          "teacher_init_conf", "teacher_aligned", "teacher_aligned_conf", "teacher_refined", "teacher_refined_conf")


def panel_names(outs, image2=None):
    """Which of the thirteen panels `_visualise` draws for these `net_outs`, in strip order (base_trainer.py:118-187)."""
    names = ["image", "ground_truth"]
    if "teacher_labels" in outs:
        names.append("teacher_labels")
    names += ["prediction", "confidence"]
    if image2 is not None:
        names.append("image2")
    if "teacher_conf" in outs:
        names.append("teacher_conf")
    for key in ("teacher_init", "teacher_aligned", "teacher_refined"):
        if key in outs:
            names += [key, key + "_conf"]
    return names


_tables = {}


def _device_table(array, dtype, device):
    array = np.ascontiguousarray(np.asarray(array, dtype=dtype))
    key = (array.tobytes(), str(dtype), device)
    if key not in _tables:
        if len(_tables) > 16:
            _tables.clear()
        _tables[key] = torch.from_numpy(array.copy()).to(device)
    return _tables[key]


def render(image, masks_gt, outs, im_size=IM_SIZE, image2=None, mean=MEAN, std=STD, palette=None, cmap=None, want_u8=False):
    """The panel strip of one batch: float32 [B,3,h,P*w] on the device (the reference's `visuals`), P = len(panel_names(outs,
    image2)); with want_u8 also the u8 rows `_visualise_grid` makes of it.  image / image2 [B,3,H,W] normalised frames, masks_gt
    int64 [B,H,W] as the forward pass left it (-1 already 255: sac.py:337-338), outs the `net_outs` of that pass.  palette u8
    [256,3] (default CS_PALETTE), cmap float32 [256,3] (default colormap("inferno")).  One launch; `outs`, `image`, `masks_gt`
    are not modified."""
    from dasac_hip import ops
    names = panel_names(outs, image2)
    col = {n: i for i, n in enumerate(names)}
    if "teacher_init" in outs and image2 is None:
        raise ValueError("render: `teacher_init` is drawn over image2 (base_trainer.py:169); pass image2")
    if "teacher_aligned" in outs and "frames_aligned" not in outs:
        raise ValueError("render: `teacher_aligned` is drawn over outs['frames_aligned'] (base_trainer.py:172)")
    jobs = [(ops.VIS_IMAGE, image, None, False, col["image"], 0),
            (ops.VIS_LABELS, masks_gt, image, False, col["ground_truth"], 0)]
    if "teacher_labels" in outs:
        jobs.append((ops.VIS_LABELS, outs["teacher_labels"], image, False, col["teacher_labels"], 0))
    jobs.append((ops.VIS_SCORES, outs["logits_up"], image, True, col["prediction"], col["confidence"]))
    if image2 is not None:
        jobs.append((ops.VIS_IMAGE, image2, None, False, col["image2"], 0))
    if "teacher_conf" in outs:
        jobs.append((ops.VIS_CONF, outs["teacher_conf"], image, False, col["teacher_conf"], 0))
    for key, back, softmax in (("teacher_init", image2, True), ("teacher_aligned", outs.get("frames_aligned"), False),
                               ("teacher_refined", image, False)):
        if key in outs:
            jobs.append((ops.VIS_SCORES, outs[key], back, softmax, col[key], col[key + "_conf"]))
    device = image.device
    pal = _device_table(CS_PALETTE if palette is None else palette, np.uint8, device)
    cm = _device_table(colormap("inferno") if cmap is None else cmap, np.float32, device)
    return ops.vis_panels(jobs, im_size, len(names), mean, std, pal, cm, want_u8=want_u8)


def grid_shape(batch, h, wt, padding=GRID_PADDING):
    """[3, rows, cols] of `to_grid`: a single row stays as it is."""
    return (3, h, wt) if batch == 1 else (3, batch * (h + padding) + padding, wt + padding)


def to_grid(rows, padding=GRID_PADDING, pad_value=GRID_PAD_VALUE):
    """`_visualise_grid` (base_trainer.py:258-270): the rows of a batch quantised with `.mul(255).clamp(0, 255).byte()` and
    stacked like make_grid(nrow=1, padding=8, pad_value=0.9): for more than one row a u8 [3, B*(h+8)+8, W+8] image filled with
    trunc(0.9 * 255) = 229, row k at y = k*(h+8)+8, x = 8; a single row is returned unpadded.  `rows`: the float32 strip on the
    device (one kernel quantises and places it) or u8 rows [B,3,h,W] on any device (placement only, e.g. after gather_rows)."""
    if rows.dtype != torch.uint8:
        from dasac_hip import ops
        return ops.vis_grid(rows, padding, pad_value)
    B, ch, h, wt = rows.shape
    if B == 1:
        return rows[0].clone()
    grid = rows.new_full(grid_shape(B, h, wt, padding), int(min(max(pad_value * 255.0, 0.0), 255.0)))
    for k in range(B):
        y = k * (h + padding) + padding
        grid[:, y:y + h, padding:padding + wt].copy_(rows[k])
    return grid


def gather_rows(rows, running_conf=None):
    """The reference's `gather_cpu` (base_trainer.py:78-95) applied to the RENDERED rows instead of `net_outs`: every rank's
    rows concatenated along the batch, rank-major, plus the class prior as `_visualise` logs it -- `running_conf` gathered and
    `view(-1, C).mean(0)` (:193-198), a list of C floats (None without running_conf).  Every rank gets both.  RCCL gathers the
    device tensors; gloo is a host transport that reads device memory with no ordering against the stream that fills it
    (driver.prep_batch), so under gloo the HOST tensors are exchanged."""
    import torch.distributed as dist
    multi = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    C = None if running_conf is None else running_conf.shape[-1]
    if multi:
        if dist.get_backend() == "gloo":
            rows = rows.cpu()
            running_conf = None if running_conf is None else running_conf.detach().cpu()
        rows = rows.contiguous()
        parts = [torch.empty_like(rows) for _ in range(dist.get_world_size())]
        dist.all_gather(parts, rows)
        rows = torch.cat(parts, 0)
        if running_conf is not None:
            running_conf = running_conf.detach().contiguous()
            parts = [torch.empty_like(running_conf) for _ in range(dist.get_world_size())]
            dist.all_gather(parts, running_conf)
            running_conf = torch.cat(parts, 0)
    confs = None
    if running_conf is not None:
        confs = running_conf.detach().cpu().view(-1, C).mean(0).tolist()
    return rows, confs


class FixedBatches(object):
    """The fixed-batch cache of `BaseTrainer` (base_trainer.py:200-218): host clones of one batch per tag, the batch every
    epoch's summary is drawn from."""

    def __init__(self):
        self.fixed_batch = None

    def save_fixed_batch(self, key, batch):
        if self.fixed_batch is None:
            self.fixed_batch = {}
        if key in self.fixed_batch:
            print("Updating fixed batch: ", key)
        self.fixed_batch[key] = [el.clone().cpu() if torch.is_tensor(el) else el for el in batch]

    def has_fixed_batch(self, key):
        return self.fixed_batch is not None and key in self.fixed_batch

    def __getitem__(self, key):
        return self.fixed_batch[key]
