"""Golden vectors of the epoch summary panels (g20).  Runs ONLY in the build container (needs the reference):

    cd <repo> && python -B tests/golden/make_goldens_visualise.py

The reference's OWN code runs on CPU: `train.py` is imported behind the stand-in modules of make_goldens_validation.py, and
`Trainer._visualise` (base_trainer.py:75-198) is called unbound on a stub `self` with its helpers `_apply_cmap`, `_error_rgb`,
`_mask_rgb` bound to the same stub, a one-rank gloo group under its `all_gather`, `Tensor.cuda` a no-op.  `_visualise_grid`
itself cannot run here (it uses `np.float`, gone from NumPy >= 1.24, and `make_grid` of the absent torchvision): it is replaced
by an OBSERVER that keeps `visuals` -- the float strip -- and quantises it with the reference's one expression
(`.mul(255).clamp(0, 255).byte()`, :264).  Only data goes into the file.

`outs` comes from a real `SAC.forward(..., use_teacher=True)` of the reference (student / teacher weights from
`oracle.nets_ref.resnet101_state`, as in g19) on B = 2 views of H x W = 33 x 41, so the keys, shapes and dtypes are the
reference's own.  What was done to keep the file below 1 MB: the frames are blocky (4 x 4 blocks of colours on a 1/16 grid,
normalised) so that they compress; every float tensor of `outs` is rounded to the nearest float16-representable value BEFORE it
is handed to `_visualise` and stored as float16 (the test widens it back: bit-equal inputs on both sides); label maps are
stored as uint8 (after the forward pass rewrote -1 to 255); the source pass reuses the student's `logits_up` of the same frames
(asserted equal to a real `net(image, gt)` source forward, so it is stored once).  Runs:
    shrink    the full 33 x 41 tensors to TB.IM_SIZE = (20, 28), which neither divides nor equals the input;
    enlarge   the window [5:17, 7:22] (12 x 15) of every tensor to (17, 23) -- the test cuts the same window.
each for the source pass (4 panels) and the target pass (13 panels).

Per pixel of every score read (prediction, teacher_init, teacher_aligned, teacher_refined) two margins, float16, in units of
their bounds and clipped at MARGIN_CAP: `<run>_<panel>_gap` = top-2 gap of the resized scores / EPS, `<run>_<panel>_frac` =
|256 (1 - conf) - nearest integer| / (256 EPS), the latter also for `teacher_conf`.  A class-overlay pixel is exempt when gap < 1;
a confidence-overlay pixel when frac <= 1 or gap < 1.  The generator asserts that at most MAX_EXEMPT of any panel is exempt.

Also stored: the palette bytes obtained from `CSPalette()` through `_apply_cmap` (Pillow) on a map of all 256 indices, the
inferno table, and `_apply_cmap` of a hand-made label map holding -1, 19, 254, 255 and 300 (the saturation rule)."""
import functools
import os
import socket
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens_validation as GV  # noqa: E402  (imports the reference's train.py on CPU behind the stand-in modules)

ref_train, ref_cfg, MG, nets_ref = GV.ref_train, GV.ref_cfg, GV.MG, GV.nets_ref
from tools.category import CSPalette  # noqa: E402  (reference)

H, W, N, T = 33, 41, 1, 2
STUDENT_SEED, TEACHER_SEED, DATA_SEED = 19, 23, 2000
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]          # datasets/dataloader_base.py:39-40
EPS, MARGIN_CAP, MAX_EXEMPT = 2e-5, 8.0, 0.03
RUN_CONF_UPPER = 0.75      # MODEL.RUN_CONF_UPPER of the shipped configuration
RUNS = {"shrink": (None, (20, 28)), "enlarge": ((5, 17, 7, 22), (17, 23))}
SCORE_READS = (("prediction", "logits_up", True), ("teacher_init", "teacher_init", True), ("teacher_aligned", "teacher_aligned", False),
               ("teacher_refined", "teacher_refined", False))
# identity and flip only: both views cover the whole reference frame and each other, so neither `teacher_aligned` nor
# `teacher_refined` has all-zero pixels (whose arg-max is a 19-way tie: exempt pixels, capped at MAX_EXEMPT of a panel)
VIEW_PARAMS = [GV.VIEW_PARAMS[0], GV.VIEW_PARAMS[3]]


def view_affines():
    from datasets.dataloader_target import DataTarget
    ref_cfg.DATASET.CROP_SIZE = [H, W]
    ref_cfg.TRAIN.GROUP_SIZE = T

    class _Shim:
        cfg = ref_cfg
    aff = DataTarget._get_affine(_Shim, VIEW_PARAMS)
    inv = DataTarget._get_affine_inv(_Shim, aff, VIEW_PARAMS)
    ref_cfg.DATASET.CROP_SIZE = [512, 1024]
    return aff.repeat(N, 1, 1), inv.repeat(N, 1, 1)


def frames(gen):
    """Blocky colour images in [0, 1] on a 1/16 grid, normalised like the loaders do."""
    rgb = (0.5 + 0.3 * GV.blocky(gen, (N * T, 3, H, W))).clamp(0, 1)
    rgb = (rgb * 16).round() / 16
    shifted = (rgb + GV.blocky(gen, (N * T, 3, 1, 1), 1) / 8).clamp(0, 1)          # a per-view, per-channel brightness shift
    mean, std = torch.tensor(MEAN).view(1, 3, 1, 1), torch.tensor(STD).view(1, 3, 1, 1)
    return (shifted - mean) / std, (rgb - mean) / std


def ground_truth(gen, maps_a, maps_b):
    """6 x 6 blocks of the teacher's arg-max (40 %), the student's (25 %), a random class (25 %), 255 (10 %); one strip with every class."""
    bh, bw = (H + 5) // 6, (W + 5) // 6
    grow = lambda t: t.repeat_interleave(6, 1).repeat_interleave(6, 2)[:, :H, :W]
    pick = grow(torch.rand(N * T, bh, bw, generator=gen))
    rnd = grow(torch.randint(0, 19, (N * T, bh, bw), generator=gen))
    gt = torch.where(pick < 0.40, maps_a, torch.where(pick < 0.65, maps_b, rnd))
    gt[pick >= 0.90] = 255
    gt[0, 10, :19] = torch.arange(19)
    gt[1, 8, 9:28] = torch.arange(19)                  # inside the window of the enlarging run too
    return gt.contiguous()


def window(t, win):
    if win is None or not torch.is_tensor(t) or t.dim() < 3:
        return t
    y0, y1, x0, x1 = win
    return t[..., y0:y1, x0:x1].contiguous()


class Observer:
    """Stands where `_visualise_grid` and the TensorBoard writer stand."""

    def __init__(self):
        self.strip, self.scalars = None, []

    def grid(self, writer, x_all, t, tag, ious=None, scores=None):
        self.strip = x_all.clone()

    def add_scalar(self, key, val, step):
        self.scalars.append((key, val))


def run_visualise(stub, image, gt, outs, im_size, image2=None):
    obs = Observer()
    stub._visualise_grid = obs.grid
    ref_cfg.TB.IM_SIZE = tuple(im_size)
    ref_train.Trainer._visualise(stub, 0, image.clone(), gt.clone(), dict(outs), obs, "tag", image2=None if image2 is None else image2.clone())
    strip = obs.strip
    assert strip.dtype == torch.float32
    rows = strip.mul(255).clamp(0, 255).byte()         # base_trainer.py:264, the reference's one expression
    return strip, rows, obs.scalars


def margins(scores, softmax, im_size):
    """(gap / EPS, frac / (256 EPS)) of one score read, by the reference's own arithmetic (base_trainer.py:152-165)."""
    if softmax:
        scores = F.softmax(scores, 1)
    p = F.interpolate(scores.float(), tuple(im_size), mode="bilinear", align_corners=True)
    conf = p.max(1)[0]
    return GV.top2_gap(p) / EPS, frac_margin(conf)


def frac_margin(conf):
    xa = ((1 - conf) * 256).double()                   # float32 product, as matplotlib computes it on a float32 array
    return (xa - xa.round()).abs().float() / (256 * EPS)


def f16(t):
    return t.clamp(max=MARGIN_CAP).to(torch.float16).numpy()


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    import torch.distributed as dist
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=0, world_size=1)
    torch.Tensor.cuda = lambda self, *a, **k: self

    net = MG.make_sac(RUN_CONF_UPPER=RUN_CONF_UPPER)
    net.backbone.load_state_dict(nets_ref.resnet101_state(seed=STUDENT_SEED, **GV.STATE_KW), strict=True)
    net.slow_net.load_state_dict(nets_ref.resnet101_state(seed=TEACHER_SEED, **GV.STATE_KW), strict=True)
    net.slow_init[0] = True
    net.eval()
    ref_cfg.TRAIN.NUM_GROUPS, ref_cfg.TRAIN.GROUP_SIZE = N, T

    palette = CSPalette()
    stub = types.SimpleNamespace(cfg=ref_cfg, world_size=1, main_process=True,
                                 loader_source=types.SimpleNamespace(dataset=types.SimpleNamespace(get_palette=lambda: palette)))
    from datasets.dataloader_seg import DLSeg
    stub.denorm = functools.partial(DLSeg.denorm, types.SimpleNamespace(MEAN=MEAN, STD=STD))
    for name in ("_apply_cmap", "_error_rgb", "_mask_rgb"):
        setattr(stub, name, functools.partial(getattr(ref_train.Trainer, name), stub))

    gen = torch.Generator().manual_seed(DATA_SEED)
    aff, inv = view_affines()
    with torch.no_grad():
        f1, f2 = frames(gen)
        tea_logits = net.slow_net(f2)[1]
        net.running_conf.copy_(torch.softmax(tea_logits, 1).mean(0).view(19, -1).mean(-1))          # what the first update would store
        gt = ground_truth(gen, tea_logits.argmax(1), net.backbone(f1)[1].argmax(1))
        gt[1, :8, -1:] = -1                            # augmentation padding (dataloader_target.py): its scores are all zero, a
        gt[0, :1, :12] = -1                            # 19-way tie -- kept small, exempt pixels are capped
        gt_in = gt.clone()
        _, outs = net(f1, gt, f2, aff, inv, use_teacher=True, update_teacher=False, T=T)       # rewrites -1 to 255 in gt
        gt_src = gt_in.clone()
        _, outs_src = net(f1, gt_src)
    assert torch.equal(gt, gt_src) and (gt_in == -1).any() and not (gt == -1).any()
    assert torch.equal(outs_src["logits_up"], outs["logits_up"])          # eval mode: the source pass sees the same student
    print("net_outs:", {k: (tuple(v.shape), str(v.dtype)) for k, v in outs.items() if torch.is_tensor(v)})
    print("source net_outs:", sorted(outs_src))

    # float tensors rounded to float16-representable values: what both sides get
    outs = {k: (v.detach().half().float() if torch.is_tensor(v) and v.is_floating_point() and k != "running_conf" else v) for k, v in outs.items()}
    outs_src = {k: outs[k] for k in outs_src}
    rec = dict(H=H, W=W, B=N * T, eps=EPS, margin_cap=MARGIN_CAP, max_exempt=MAX_EXEMPT, mean=np.array(MEAN, np.float32),
               std=np.array(STD, np.float32), image=f1, image2=f2, gt_loaded=gt_in.to(torch.int16), masks_gt=gt.to(torch.uint8),
               running_conf=outs["running_conf"].clone(), runs=np.array(sorted(RUNS)),
               target_keys=np.array([k for k in outs if torch.is_tensor(outs[k])]), source_keys=np.array(sorted(outs_src)))
    for k, v in outs.items():
        if not torch.is_tensor(v) or k == "running_conf":
            continue
        if v.is_floating_point():
            assert torch.equal(v.half().float(), v)
            rec["out_" + k] = v.half()
        else:
            assert int(v.min()) >= 0 and int(v.max()) <= 255, k
            rec["out_" + k] = v.to(torch.uint8)

    for run, (win, im_size) in RUNS.items():
        cut = lambda t: window(t, win)
        o_t, o_s = {k: cut(v) for k, v in outs.items()}, {k: cut(v) for k, v in outs_src.items()}
        rec[run + "_size"] = np.array(im_size)
        rec[run + "_window"] = np.array(win if win is not None else (0, H, 0, W))
        for name, o, image2 in (("source", o_s, None), ("target", o_t, cut(f2))):
            strip, rows, scalars = run_visualise(stub, cut(f1), cut(gt), o, im_size, image2)
            P = 4 if name == "source" else 13
            assert tuple(strip.shape) == (N * T, 3, im_size[0], P * im_size[1]), strip.shape
            assert float(strip.min()) >= -1e-3 and float(strip.max()) <= 1 + 1e-3, (float(strip.min()), float(strip.max()))
            rec["%s_%s_strip" % (run, name)], rec["%s_%s_rows" % (run, name)] = strip, rows
            if name == "target":
                rec[run + "_running_conf_logged"] = np.array([v for _, v in scalars], np.float64)
                assert len(scalars) == 19
        for panel, key, softmax in SCORE_READS:
            gap, frac = margins(o_t[key], softmax, im_size)
            rec["%s_%s_gap" % (run, panel)], rec["%s_%s_frac" % (run, panel)] = f16(gap), f16(frac)
            ex_class, ex_conf = gap < 1, (frac <= 1) | (gap < 1)
            print("{:8s} {:16s} exempt: class {:.4f} confidence {:.4f}".format(run, panel, float(ex_class.float().mean()), float(ex_conf.float().mean())))
            assert float(ex_class.float().mean()) <= MAX_EXEMPT and float(ex_conf.float().mean()) <= MAX_EXEMPT, (run, panel)
        tc = F.interpolate(o_t["teacher_conf"].float(), tuple(im_size), mode="bilinear", align_corners=True)[:, 0]
        frac = frac_margin(tc)
        rec[run + "_teacher_conf_frac"] = f16(frac)
        print("{:8s} {:16s} exempt: confidence {:.4f}".format(run, "teacher_conf", float((frac <= 1).float().mean())))
        assert float((frac <= 1).float().mean()) <= MAX_EXEMPT

    # ---- palette, colour map, saturation -----------------------------------------------------------------
    every = torch.arange(256).view(1, 16, 16)
    pal = (ref_train.Trainer._apply_cmap(stub, every, palette)[0] * 255).round().to(torch.uint8).permute(1, 2, 0).reshape(256, 3)
    rec["palette"] = pal
    odd = torch.tensor([[[-1, 19, 254, 255, 300, 0, 18, 7]]])
    rec["saturation_labels"] = odd.to(torch.int32)
    rec["saturation_rgb"] = (ref_train.Trainer._apply_cmap(stub, odd, palette)[0] * 255).round().to(torch.uint8).permute(1, 2, 0).reshape(-1, 3)
    from matplotlib import cm
    inferno = cm.get_cmap("inferno")
    rec["inferno"] = np.asarray(inferno(np.arange(256))[:, :3], np.float64)
    probe = np.array([0.0, 0.5, 255.5 / 256, 1.0, 1.5, -0.25], np.float32)
    rec["inferno_probe"], rec["inferno_probe_rgb"] = probe, np.asarray(inferno(probe)[:, :3], np.float64)

    # ---- the conditions that keep the tests from passing vacuously ------------------------------------------
    for run, (win, _) in RUNS.items():
        g = window(gt, win).numpy()
        present = set(np.unique(g))
        print(run, "values in the ground truth:", len(present))
        assert present >= set(range(19)) | {255}, sorted(present)
        share = float((window(outs["teacher_labels"], win) != 255).float().mean())
        print(run, "labelled share of teacher_labels: {:.3f}".format(share))
        assert 0.20 <= share <= 0.80, share
        w = RUNS[run][1][1]
        panel = lambda i: rec[run + "_target_strip"][..., i * w:(i + 1) * w]
        assert not torch.equal(panel(7), panel(9)) and not torch.equal(panel(9), panel(11)) and not torch.equal(panel(7), panel(11))
        maps = [F.interpolate((F.softmax(window(outs[k], win), 1) if sm else window(outs[k], win)), RUNS[run][1], mode="bilinear",
                              align_corners=True).argmax(1) for _, k, sm in SCORE_READS[1:]]
        differ = [float((maps[i] != maps[j]).float().mean()) for i, j in ((0, 1), (1, 2), (0, 2))]
        print(run, "teacher class maps differ on", differ)
        assert min(differ) > 0.01, differ

    out = {}
    for k, v in rec.items():
        out[k] = np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v)
    path = os.path.join(HERE, "g20_visualise.npz")
    GV.write_npz(path, out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
