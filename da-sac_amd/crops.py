"""Source crops and the target front half on the device (continued) -- the pixel work in front of
`views.TargetViews`:

    source loader DLSeg      /root/reference/datasets/dataloader_seg.py:70-113,141-161
        train: ["game" pre-resize to 1914x1052], MaskRandScale (tf_seg.py:129-153), [RandGaussianBlur(1.0) :213-227],
               [MaskRandHFlip :202-211], [MaskRandJitter(RND_JITTER) :229-247], MaskRandCrop(pad_if_needed) :155-187
        eval:  MaskCenterCrop (:189-200) or MaskScale (:115-127)
        then ToTensorMask / Normalize / ApplyMask(255) (:33-89)
    target loader DataTarget.tf_pre   dataloader_target.py:101-107
        MaskScale(CROP_SIZE) (tf_target.py:127-139), MaskRandScale(TARGET_SCALE) (:241-263), MaskRandCrop(pad_if_needed)
        (:265-303), [MaskRandHFlip :318-329, after the crop], then what views.TargetViews does; eval: MaskCenterCrop / MaskScale
        and ApplyMask(-1)

The loader hands over the decoded u8 images (HWC, as they come from the decoder) and u8 labels; B images of any sizes are
packed back to back and moved with one H2D copy.  Without a photometric op in between the whole source batch is ONE
launch (dasac_make_crops: resample-or-copy, flip, pad, crop, normalise, mask per output pixel).  Resizes whose result
something else must see whole -- the game pre-resize, the target's MaskScale, the scaled image under the source blur /
jitter -- go through dasac_resize_u8 first (Pillow rounds every resize to u8, so two resizes are never folded into one).

Draws follow the reference's call order on a `random.Random` (its module-level `random`) and a `torch.Generator` (its global
torch RNG: RandomCrop.get_params and ColorJitter.get_params).  torchvision is not a dependency; its semantics are restated
for torchvision >= 0.8, the version views.sample_photometric assumes:
    RandomCrop.get_params   (0, 0, h, w) with NO draw when the padded size equals the crop size, else
                            i = torch.randint(0, h - th + 1, (1,)), then j the same way;
    ColorJitter.get_params  torch.randperm(4), then a uniform per enabled factor (brightness, contrast, saturation in
                            [max(0, 1 - j), 1 + j], hue in [-h, h]); a factor of 0 is disabled and draws nothing;
    center_crop             top = int(round((h - th) / 2.0)), left likewise (python's round: half to even).
"""
import random

import numpy as np
import torch

from dasac_hip import lib as L
import views

MEAN, STD = views.MEAN, views.STD
DESC = 16                               # int64 per descriptor row (include/dasac_hip.h: DASAC_CROP_DESC)
GAME_SIZE = (1052, 1914)                # dataloader_seg.py:150-152: (w, h) = (1914, 1052)
FLIP_NONE, FLIP_BEFORE_CROP, FLIP_AFTER_CROP = 0, 1, 2


# ------------------------------------------------------------------------------------------------
# draws, in the reference's order (no pixel work: tests inject or compare them)
# ------------------------------------------------------------------------------------------------
def _crop_params(torch_gen, padded_hw, crop_hw):
    """RandomCrop.get_params (torchvision >= 0.8) on the padded image."""
    (h, w), (th, tw) = padded_hw, crop_hw
    if h == th and w == tw:
        return 0, 0
    i = int(torch.randint(0, h - th + 1, (1,), generator=torch_gen))
    j = int(torch.randint(0, w - tw + 1, (1,), generator=torch_gen))
    return i, j


def _pad(scaled_hw, crop_hw):
    """MaskRandCrop.__pad (tf_seg.py:163-176): (pad_t, pad_l) and the padded size; pad_r / pad_b take the odd pixel."""
    (sh, sw), (th, tw) = scaled_hw, crop_hw
    ph, pw = max(0, th - sh), max(0, tw - sw)
    return (ph // 2, pw // 2), (sh + ph, sw + pw)


def _scaled(hw, s):
    """MaskRandScale: PIL size (int(w * s), int(h * s)) -- returned as (h, w)."""
    return int(hw[0] * s), int(hw[1] * s)


def sample_jitter(rng, torch_gen, jitter, hue_max):
    """MaskRandJitter.__call__: `random.random() < 0.5`, then ColorJitter.get_params.  Returns (order, factors) or None;
    a disabled factor is None."""
    if not rng.random() < 0.5:
        return None
    order = torch.randperm(4, generator=torch_gen).tolist()
    lo, hi, hue = max(0., 1. - jitter), 1. + jitter, min(hue_max, jitter)
    fac = [float(torch.empty(1).uniform_(lo, hi, generator=torch_gen)) if jitter > 0 else None for _ in range(3)]
    fac.append(float(torch.empty(1).uniform_(-hue, hue, generator=torch_gen)) if hue > 0 else None)
    return order, fac


def sample_source(rng, torch_gen, hw, crop_hw, scale_range=(0.5, 1.0), blur=False, hflip=True, jitter=None):
    """DLSeg's train chain for one image of size hw = (H, W) (after the game pre-resize): MaskRandScale, [RandGaussianBlur],
    [MaskRandHFlip], [MaskRandJitter(jitter)], MaskRandCrop(pad_if_needed).  `jitter` None = no MaskRandJitter in the chain
    (SRC_RND_JITTER == 0), else its strength (RND_JITTER).  Returns a dict: scale, scaled (h, w), blur, flip, jitter
    ((order, factors) or None), pad (t, l), crop (i, j)."""
    a, b = scale_range
    s = a + (b - a) * rng.random()
    d = dict(scale=s, scaled=_scaled(hw, s), blur=False, flip=False, jitter=None)
    if blur:
        d["blur"] = rng.random() < 0.5
    if hflip:
        d["flip"] = rng.random() > 0.5
    if jitter is not None:
        d["jitter"] = sample_jitter(rng, torch_gen, float(jitter), 0.5)
    d["pad"], padded = _pad(d["scaled"], crop_hw)
    d["crop"] = _crop_params(torch_gen, padded, crop_hw)
    return d


def sample_target_front(rng, torch_gen, crop_hw, target_scale=(1.0, 1.1), hflip=True):
    """DataTarget.tf_pre's draws up to the views (after MaskScale(crop_hw), which draws nothing): MaskRandScale, MaskRandCrop,
    [MaskRandHFlip].  Returns a dict: scale, scaled (h, w), pad (t, l), crop (i, j), flip."""
    a, b = target_scale
    s = a + (b - a) * rng.random()
    d = dict(scale=s, scaled=_scaled(crop_hw, s))
    d["pad"], padded = _pad(d["scaled"], crop_hw)
    d["crop"] = _crop_params(torch_gen, padded, crop_hw)
    d["flip"] = bool(hflip) and rng.random() > 0.5
    return d


def center_crop_params(hw, crop_hw):
    """torchvision center_crop of an image at least as large as the crop: (top, left)."""
    (h, w), (th, tw) = hw, crop_hw
    if h < th or w < tw:
        raise NotImplementedError("center crop {} of a smaller {}x{} image (torchvision pads there; not supported)".format(crop_hw, h, w))
    return int(round((h - th) / 2.0)), int(round((w - tw) / 2.0))


# ------------------------------------------------------------------------------------------------
# tables and descriptors
# ------------------------------------------------------------------------------------------------
def table_ints(SH, SW):
    """int32 per scaled image (= dasac_crop_table_ints)."""
    return (2 + views._KS) * (SH + SW) + SH + SW


def resize_tables(hw, scaled_hw):
    """Pillow resize tables of (H, W) -> (SH, SW): bounds_h, coeff_h, bounds_v, coeff_v, nearest_x, nearest_y as one int32
    vector (views._bilinear_tables / views._nearest_table, double precision).  An unchanged axis gets identity tables, which
    reproduce Pillow's single pass.  NotImplementedError where a scale needs more than 8 taps."""
    (H, W), (SH, SW) = hw, scaled_hw
    bh, kh = views._bilinear_tables(W, SW)
    bv, kv = views._bilinear_tables(H, SH)
    parts = (bh, kh, bv, kv, views._nearest_table(W, SW), views._nearest_table(H, SH))
    out = np.concatenate([p.reshape(-1) for p in parts]).astype(np.int32)
    assert out.size == table_ints(SH, SW)
    return out


class _Batch:
    """Descriptor rows + tables of one launch; `add` returns the row."""

    def __init__(self):
        self.rows, self.tables, self.n_tab = [], [], 0

    def add(self, img_off, lab_off, hw, strides, scaled_hw, flip=0, pad=(0, 0), crop=(0, 0), out=(0, 0)):
        H, W = hw
        SH, SW = scaled_hw
        if (SH, SW) == (H, W):
            tab = -1                     # Image.resize to the same size is a copy
        else:
            t = resize_tables(hw, scaled_hw)
            tab = self.n_tab
            self.tables.append(t)
            self.n_tab += t.size
        self.rows.append([img_off, lab_off, H, W, strides[0], strides[1], SH, SW, tab, flip, pad[0], pad[1], crop[0], crop[1],
                          out[0], out[1]])

    def upload(self, dev):
        desc = torch.tensor(self.rows, dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
        tab = np.concatenate(self.tables) if self.tables else np.zeros(1, np.int32)
        tab = torch.from_numpy(tab).pin_memory().to(dev, non_blocking=True)
        return desc, tab, self.n_tab


class _Packed:
    """B images (+ labels) in two flat u8 device buffers with per-image offsets and strides."""

    def __init__(self, img, lab, offsets, hws, strides):
        self.img, self.lab, self.offsets, self.hws, self.strides = img, lab, offsets, hws, strides


def pack(images, labels, dev, fill_label=0):
    """HWC u8 images [H,W,3] and u8 labels [H,W] (None: an all-`fill_label` label) -> one packed buffer each, with one H2D
    copy per buffer for host inputs."""
    assert len(images) == len(labels) and len(images) > 0
    hws, offs, o_img, o_lab = [], [], 0, 0
    for im, lb in zip(images, labels):
        if im.dim() != 3 or im.shape[2] != 3 or im.dtype != torch.uint8:
            raise ValueError("images must be HWC uint8 [H,W,3], got {} {}".format(tuple(im.shape), im.dtype))
        H, W = int(im.shape[0]), int(im.shape[1])
        if lb is not None and (tuple(lb.shape) != (H, W) or lb.dtype != torch.uint8):
            raise ValueError("label must be uint8 [H,W] = {}, got {} {}".format((H, W), tuple(lb.shape), lb.dtype))
        hws.append((H, W))
        offs.append((o_img, o_lab))
        o_img += 3 * H * W
        o_lab += H * W

    def flat(ts, n, host):
        buf = torch.empty(n, dtype=torch.uint8, pin_memory=host) if host else torch.empty(n, dtype=torch.uint8, device=dev)
        o = 0
        for t in ts:
            buf[o:o + t.numel()].copy_(t.reshape(-1))
            o += t.numel()
        return buf.to(dev, non_blocking=True) if host else buf
    host = not images[0].is_cuda
    labs = [lb if lb is not None else torch.full((h, w), fill_label, dtype=torch.uint8, device=images[0].device)
            for lb, (h, w) in zip(labels, hws)]
    for t in list(images) + labs:
        if t.is_cuda == host:
            raise ValueError("images and labels must all be on the host or all on the device")
    return _Packed(flat(images, o_img, host), flat(labs, o_lab, host), offs, hws, [(3, 1)] * len(hws))


def resize(src, sizes):
    """dasac_resize_u8: every image of `src` to sizes[b] = (SH, SW) -> a new planar _Packed."""
    lib, dev = L.load(), src.img.device
    bt, o_img, o_lab, offs = _Batch(), 0, 0, []
    for b, ((H, W), (SH, SW)) in enumerate(zip(src.hws, sizes)):
        bt.add(src.offsets[b][0], src.offsets[b][1], (H, W), src.strides[b], (SH, SW), out=(o_img, o_lab))
        offs.append((o_img, o_lab))
        o_img += 3 * SH * SW
        o_lab += SH * SW
    desc, tab, n_tab = bt.upload(dev)
    out_img = torch.empty(o_img, dtype=torch.uint8, device=dev)
    out_lab = torch.empty(o_lab, dtype=torch.uint8, device=dev)
    L.check(lib.dasac_resize_u8(src.img.data_ptr(), src.img.numel(), src.lab.data_ptr(), src.lab.numel(), len(sizes), desc.data_ptr(),
                                tab.data_ptr(), n_tab, max(h * w for h, w in sizes), out_img.data_ptr(), out_img.numel(), out_lab.data_ptr(),
                                out_lab.numel(), L.stream_ptr()), "dasac_resize_u8")
    return _Packed(out_img, out_lab, offs, [tuple(s) for s in sizes], [(1, h * w) for h, w in sizes])


def make_crops(src, crops, crop_hw, mean, std, ignore_label, want=("frames", "labels")):
    """dasac_make_crops over the packed images: crops[b] = dict(scaled, flip, pad, crop).  Returns the requested outputs
    among frames f32 [B,3,Hc,Wc], labels i64 [B,Hc,Wc], image_u8, label_u8, mask_u8."""
    lib, dev = L.load(), src.img.device
    Hc, Wc = crop_hw
    B = len(crops)
    bt = _Batch()
    for b, c in enumerate(crops):
        SH, SW = c["scaled"]
        pt, pl = c["pad"]
        ci, cj = c["crop"]
        if ci < 0 or cj < 0 or ci + Hc > max(SH, Hc) or cj + Wc > max(SW, Wc):
            raise ValueError("crop {} outside the padded {}x{} image".format(c["crop"], SH, SW))
        bt.add(src.offsets[b][0], src.offsets[b][1], src.hws[b], src.strides[b], (SH, SW), c["flip"], (pt, pl), (ci, cj))
    desc, tab, n_tab = bt.upload(dev)
    shapes = dict(frames=((B, 3, Hc, Wc), torch.float32), labels=((B, Hc, Wc), torch.int64), image_u8=((B, 3, Hc, Wc), torch.uint8),
                  label_u8=((B, Hc, Wc), torch.uint8), mask_u8=((B, Hc, Wc), torch.uint8))
    out = {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=dev) for k in want}
    get = lambda k: L.ptr(out.get(k))
    m, s = np.asarray(mean, dtype=np.float32), np.asarray(std, dtype=np.float32)
    L.check(lib.dasac_make_crops(src.img.data_ptr(), src.img.numel(), src.lab.data_ptr(), src.lab.numel(), B, desc.data_ptr(), tab.data_ptr(),
                                 n_tab, Hc, Wc, m.ctypes.data, s.ctypes.data, int(ignore_label), get("frames"), get("labels"),
                                 get("image_u8"), get("label_u8"), get("mask_u8"), L.stream_ptr()), "dasac_make_crops")
    return tuple(out[k] for k in want)


def photometric_in_place(src, b, blur, jitter):
    """Source RandGaussianBlur(1.0) / MaskRandJitter on the whole scaled image b of a planar _Packed: dasac_view_photometric
    with L = 1 (its ABI unchanged; the f32 frames it must write go to scratch), result written back over the bytes.  The
    reference flips between blur and jitter; both commute with the flip (the box blur is symmetric with mirrored edge
    replication, the jitter's only global term is the contrast mean), so make_crops applies the flip afterwards."""
    lib, dev = L.load(), src.img.device
    H, W = src.hws[b]
    assert src.strides[b] == (1, H * W)
    row = dict(blur=1.0 if blur else None, jitter=None, grey=False)
    if jitter is not None and all(f is not None for f in jitter[1]):
        row["jitter"] = jitter
    elif jitter is not None and any(f is not None for f in jitter[1]):
        raise NotImplementedError("colour jitter with a partly disabled factor set")
    if row["blur"] is None and row["jitter"] is None:
        return
    params = np.ascontiguousarray(views.photometric_params([row]))
    mean, std = np.zeros(3, np.float32), np.ones(3, np.float32)
    frames = L.workspace(3 * H * W * 4, dev, owner="crops_photometric_frames")
    nbytes = lib.dasac_view_photometric_workspace(H, W, 1)
    ws = L.workspace(nbytes, dev)
    view = src.img[src.offsets[b][0]:src.offsets[b][0] + 3 * H * W]
    L.check(lib.dasac_view_photometric(view.data_ptr(), None, H, W, 1, params.ctypes.data, mean.ctypes.data, std.ctypes.data, -1,
                                       frames.data_ptr(), view.data_ptr(), ws.data_ptr(), nbytes, L.stream_ptr()), "dasac_view_photometric")


def _device(dev):
    if dev is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    dev = torch.device(dev)
    L.require_gpu(torch.empty(0, device=dev))
    return dev


def _renorm(cfg, mean, std):
    """DLSeg(renorm=True) (dataloader_seg.py:95-106)."""
    D = cfg.DATASET
    ms, mt, ss, st = (np.array(x, dtype=np.float64) for x in (D.SOURCE_MEAN, D.TARGET_MEAN, D.SOURCE_STD, D.TARGET_STD))
    return tuple(ms - ss / st * (mt - np.array(mean))), tuple(ss * np.array(std) / st)


# ------------------------------------------------------------------------------------------------
# the two loaders
# ------------------------------------------------------------------------------------------------
class SourceCrops:
    """DLSeg's transforms on the device.  `make(images, labels)` -> (image f32 [B,3,Hc,Wc], labels i64 [B,Hc,Wc]) -- what DLSeg
    + the default collate yield -- plus (image_u8, label_u8, mask_u8) with want_u8."""

    def __init__(self, crop_hw, train=True, scale_range=(0.5, 1.0), hflip=True, blur=False, jitter=None, val_crop=True,
                 game_size=None, mean=MEAN, std=STD, seed=None, ignore_label=255, want_u8=False):
        self.crop = (int(crop_hw[0]), int(crop_hw[1]))
        self.train, self.scale_range, self.hflip, self.blur, self.jitter = bool(train), tuple(scale_range), bool(hflip), bool(blur), jitter
        self.val_crop, self.game_size = bool(val_crop), (tuple(game_size) if game_size else None)
        self.mean, self.std, self.ignore_label, self.want_u8 = tuple(mean), tuple(std), int(ignore_label), bool(want_u8)
        self.rng = random.Random(seed)
        self.torch_gen = torch.Generator()
        self.torch_gen.manual_seed(seed if seed is not None else self.rng.getrandbits(63))

    @classmethod
    def from_cfg(cls, cfg, split, renorm=False, **kw):
        """The transforms DLSeg(cfg, split, renorm) builds (dataloader_seg.py:70-113); "game" in the split = the pre-resize."""
        D = cfg.DATASET
        train = split.startswith("train")
        if train and not D.RND_CROP:
            raise NotImplementedError("DATASET.RND_CROP = False: uncropped source images of different sizes do not batch")
        mean, std = _renorm(cfg, MEAN, STD) if renorm else (MEAN, STD)
        args = dict(train=train, scale_range=(D.SCALE_FROM, D.SCALE_TO), hflip=bool(D.RND_HFLIP), blur=bool(D.SRC_RND_BLUR),
                    jitter=D.RND_JITTER if D.SRC_RND_JITTER > 0 else None, val_crop=bool(D.VAL_CROP),
                    game_size=GAME_SIZE if "game" in split else None, mean=mean, std=std)
        args.update(kw)
        return cls(D.CROP_SIZE, **args)

    @property
    def photometric(self):
        return self.blur or self.jitter is not None

    def sample(self, hw):
        return sample_source(self.rng, self.torch_gen, hw, self.crop, self.scale_range, self.blur, self.hflip, self.jitter)

    def eval_params(self, hw):
        if self.val_crop:
            return dict(scaled=tuple(hw), flip=0, pad=(0, 0), crop=center_crop_params(hw, self.crop))
        return dict(scaled=self.crop, flip=0, pad=(0, 0), crop=(0, 0))

    def make(self, images, labels=None, params=None, device=None):
        """images: list of HWC uint8 [H,W,3] (host or device), labels: list of uint8 [H,W] or None (= all 0, as DLSeg's
        missing mask).  params: the per-image draws (`sample`) to use instead of drawing."""
        dev = images[0].device if images[0].is_cuda else _device(device)
        labels = [None] * len(images) if labels is None else list(labels)
        src = pack(list(images), labels, dev)
        if self.game_size is not None and any(hw != self.game_size for hw in src.hws):
            src = resize(src, [self.game_size] * len(images))
        if not self.train:
            crops = [self.eval_params(hw) for hw in src.hws]
        else:
            crops = [self.sample(hw) for hw in src.hws] if params is None else list(params)
            crops = [dict(c, flip=FLIP_BEFORE_CROP if c["flip"] else FLIP_NONE) for c in crops]
            if self.photometric:
                src = resize(src, [c["scaled"] for c in crops])
                for b, c in enumerate(crops):
                    photometric_in_place(src, b, c["blur"], c["jitter"])
        want = ("frames", "labels") + (("image_u8", "label_u8", "mask_u8") if self.want_u8 else ())
        return make_crops(src, crops, self.crop, self.mean, self.std, self.ignore_label, want)


class TargetCrops:
    """DataTarget's front half on the device, feeding an owned views.TargetViews with no host round trip.  Draws come from
    the TargetViews' `rng` / `torch_gen`, so one seed reproduces DataTarget.__getitem__ after the image selection -- and
    from its first line when `sampler` (a sampling.TargetSampler) is given and `select(index)` opens every sample:
    select -> front -> views consumes the python-`random` draws in DataTarget.__getitem__'s order.
    `make(image, label)` -> (frames1, gt, frames2, affine, affine_inv) as views.TargetViews.make; in eval mode
    (frames f32 [3,Hc,Wc], labels i64 [Hc,Wc]) with -1 under the padding mask."""

    IGNORE_LABEL = 255                  # dataloader_target.py:275-276: a missing label file is an all-255 label

    def __init__(self, crop_hw, group_size=4, train=True, target_scale=(1.0, 1.1), hflip=True, val_crop=False, seed=None,
                 mean=MEAN, std=STD, sampler=None, **view_kw):
        self.crop = (int(crop_hw[0]), int(crop_hw[1]))
        self.sampler = sampler
        self.train, self.target_scale, self.hflip, self.val_crop = bool(train), tuple(target_scale), bool(hflip), bool(val_crop)
        self.views = views.TargetViews(self.crop, group_size, seed=seed, mean=mean, std=std, **view_kw)
        self.mean, self.std = tuple(mean), tuple(std)

    @classmethod
    def from_cfg(cls, cfg, split, seed=None, **kw):
        """The transforms DataTarget(cfg, split) builds (dataloader_target.py:96-129)."""
        D = cfg.DATASET
        args = dict(group_size=cfg.TRAIN.GROUP_SIZE, train=not split.startswith("val"), target_scale=tuple(D.TARGET_SCALE),
                    hflip=bool(D.RND_HFLIP), val_crop=bool(D.VAL_CROP), seed=seed, zoom_range=tuple(D.RND_ZOOM),
                    guided_hflip=bool(D.GUIDED_HFLIP), blur=(.1, 2.) if D.RND_BLUR else None, jitter=float(D.RND_JITTER),
                    grey_p=float(D.RND_GREYSCALE))
        args.update(kw)
        return cls(D.CROP_SIZE, **args)

    @property
    def rng(self):
        return self.views.rng

    @property
    def torch_gen(self):
        return self.views.torch_gen

    def select(self, index):
        """The image DataTarget.__getitem__(index) opens (dataloader_target.py:264-273): one `uniform` draw from this
        object's own `rng`, before anything else of the sample."""
        if self.sampler is None:
            raise ValueError("TargetCrops.select needs a sampler (sampling.TargetSampler)")
        return self.sampler.select(index, self.rng)

    def sample(self):
        return sample_target_front(self.rng, self.torch_gen, self.crop, self.target_scale, self.hflip)

    def _scaled_to_crop(self, images, labels, dev):
        src = pack(list(images), list(labels), dev, fill_label=self.IGNORE_LABEL)
        if any(hw != self.crop for hw in src.hws):
            src = resize(src, [self.crop] * len(src.hws))          # MaskScale(CROP_SIZE): its own Pillow resize
        return src

    def front(self, images, labels=None, params=None, device=None):
        """The train front half of B images in one make_crops launch: (image_u8 [B,3,Hc,Wc], label_u8, mask_u8)."""
        dev = images[0].device if images[0].is_cuda else _device(device)
        labels = [None] * len(images) if labels is None else list(labels)
        if params is None:
            params = [self.sample() for _ in images]
        src = self._scaled_to_crop(images, labels, dev)
        crops = [dict(c, flip=FLIP_AFTER_CROP if c["flip"] else FLIP_NONE) for c in params]
        return make_crops(src, crops, self.crop, self.mean, self.std, -1, ("image_u8", "label_u8", "mask_u8"))

    def make_batch(self, images, labels=None, device=None):
        """DataTarget.__getitem__ for B images in the reference's draw order (per image: front, views, photometric) with one
        front launch; a list of B 5-tuples (eval mode: of (frames, labels))."""
        if not self.train:
            return self._eval(images, labels, device)
        draws = []
        for _ in images:
            front = self.sample()
            vs = self.views.sample()
            photo = self.views.sample_photometric() if self.views.photometric else None
            draws.append((front, vs, photo))
        img_u8, lab_u8, msk_u8 = self.front(images, labels, [d[0] for d in draws], device)
        return [self.views.make(img_u8[b], lab_u8[b], msk_u8[b], views=vs, photo=photo) for b, (_, vs, photo) in enumerate(draws)]

    def make(self, image, label=None, device=None):
        return self.make_batch([image], [label], device)[0]

    def _eval(self, images, labels, device):
        dev = images[0].device if images[0].is_cuda else _device(device)
        labels = [None] * len(images) if labels is None else list(labels)
        src = pack(list(images), labels, dev, fill_label=self.IGNORE_LABEL)
        if self.val_crop:
            crops = [dict(scaled=hw, flip=0, pad=(0, 0), crop=center_crop_params(hw, self.crop)) for hw in src.hws]
        else:
            crops = [dict(scaled=self.crop, flip=0, pad=(0, 0), crop=(0, 0)) for _ in src.hws]
        frames, gt = make_crops(src, crops, self.crop, self.mean, self.std, -1)
        return [(frames[b], gt[b]) for b in range(len(images))]

