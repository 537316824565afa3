"""Golden vectors of the reference-form validation pass (g19).  Runs ONLY in the build container (needs the reference):

    cd <repo> && python -B tests/golden/make_goldens_validation.py

The reference's OWN code runs on CPU: `Trainer.validation` with `Trainer.step` (source pass) and `Trainer._step_target` (target
pass), called unbound on a stub `self`, and `utils.metrics.Jaccard` / `utils.stat_manager.StatManager` underneath them.  Route
taken: `train.py` IS imported, after empty stand-in modules for the third-party packages it imports and this image lacks
(setproctitle, torch.utils.tensorboard, torchvision.utils) were registered in sys.modules -- the route of g11; nothing had to be
compiled out of its source.  `Tensor.cuda` is a no-op for the run (g14) and a one-rank gloo group serves `dist.all_reduce`.
The generator only OBSERVES: `Jaccard` / `StatManager` are replaced in train.py's namespace by subclasses that remember their
instances, and the step function is wrapped to keep copies of what it returned.  Only data goes into the file; the weights
come from `oracle.nets_ref.resnet101_state(seed)` on both sides (student STUDENT_SEED, teacher TEACHER_SEED), the class prior
chi is set directly and stored.

Inputs are blocky (values on a 1/8 grid in 4x4 blocks) so that they compress; the ground truth mixes the student's and the
teacher's own arg-max (the larger share the student's in the source pass, the teacher's in the target pass) with random blocks, ~10 % of 255, the augmentation padding (-1, target pass) and one strip that holds
every class.  Full layer tensors would not fit the committed-file limit (one [4,19,65,97] fp32 layer is 479 KB): the arg-max
maps and margins are stored for every counted batch, the full tensors for a window of WIN_ROWS rows of two views of two target
batches, with the counts the reference's own `Jaccard` gives on exactly those windows.

Margins (per pixel, float16, as a FRACTION of the layer's max |value| and clipped at MARGIN_CAP): arg-max layers the top-2 gap;
`teacher_labels` min(top-2 gap, |confidence - class threshold|) with the thresholds of models/sac.py:163-174 recomputed from the
stored `teacher_refined`.  The project's float contract is 1e-3 of max |value|: a pixel below it may legitimately flip.
"""
import functools
import os
import socket
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as MG  # noqa: E402  (imports the reference on CPU, registers the torchvision stand-in)

for _name in ("setproctitle", "torch.utils.tensorboard", "torchvision.utils"):
    _m = types.ModuleType(_name)
    _m.SummaryWriter = object
    sys.modules.setdefault(_name, _m)
import torchvision  # noqa: E402  (the stand-in)
torchvision.utils = sys.modules["torchvision.utils"]
import train as ref_train  # noqa: E402  (the reference's train.py)

ref_cfg, nets_ref = MG.ref_cfg, MG.nets_ref
H, W, N, T, BS = 65, 97, 1, 4, 2
NUM_BATCHES, MAX_ITER, COUNTED = 4, 1, 3
STUDENT_SEED, TEACHER_SEED, DATA_SEED = 19, 119, 1900
STATE_KW = dict(randomize_bn=True, he_init=True, residual_gain=0.25, aspp_gain=0.2)
IGNORE_SYNTHIA = [9, 14, 16]
CONTRACT, MARGIN_CAP = 1e-3, 1.0 / 16
WIN_ROWS, WIN_ROW0, WIN_VIEWS, WIN_BATCHES = 5, 30, 2, 2
SCORE_LAYERS, LABEL_LAYER = ("logits_up", "teacher_init", "teacher_refined"), "teacher_labels"
CLASS_NAMES = ["class%02d" % i for i in range(19)]


def blocky(gen, shape, block=4):
    *lead, h, w = shape
    low = torch.randn(*lead, (h + block - 1) // block, (w + block - 1) // block, generator=gen)
    x = low.repeat_interleave(block, -2).repeat_interleave(block, -1)[..., :h, :w]
    return (x * 8).round() / 8


def mixed_gt(gen, maps_a, maps_b):
    """Ground truth from two prediction maps [B,H,W]: 8x8 blocks of A (40 %), B (25 %), a random class (25 %), 255 (10 %)."""
    B = maps_a.shape[0]
    bh, bw = (H + 7) // 8, (W + 7) // 8
    pick = torch.rand(B, bh, bw, generator=gen).repeat_interleave(8, 1).repeat_interleave(8, 2)[:, :H, :W]
    rnd = torch.randint(0, 19, (B, bh, bw), generator=gen).repeat_interleave(8, 1).repeat_interleave(8, 2)[:, :H, :W]
    gt = torch.where(pick < 0.40, maps_a, torch.where(pick < 0.65, maps_b, rnd))
    gt[pick >= 0.90] = 255
    gt[0, 10, :19] = torch.arange(19)                      # every class occurs in every batch
    return gt.contiguous()


# (dy, dx, alpha, scale, flip): identity, two zoomed-in views (scale > 1: the view lies inside the reference frame), flip only --
# every pixel of every view is covered by the group, so `teacher_refined` has no all-zero pixels (whose arg-max would be a tie)
VIEW_PARAMS = [(0.0, 0.0, 0.0, 1.0, 1.0), (2.0, -3.0, 0.0, 1.25, -1.0), (-3.0, 2.0, 0.0, 1.5, 1.0), (0.0, 0.0, 0.0, 1.0, -1.0)]


def view_affines():
    """dataloader_target.py:220-262 through the reference's own (unbound) methods, as make_goldens._target_inputs does."""
    from datasets.dataloader_target import DataTarget
    ref_cfg.DATASET.CROP_SIZE = [H, W]
    ref_cfg.TRAIN.GROUP_SIZE = T

    class _Shim:
        cfg = ref_cfg
    aff = DataTarget._get_affine(_Shim, VIEW_PARAMS[:T])
    inv = DataTarget._get_affine_inv(_Shim, aff, VIEW_PARAMS[:T])
    ref_cfg.DATASET.CROP_SIZE = [512, 1024]
    return aff.repeat(N, 1, 1), inv.repeat(N, 1, 1)


class RecJaccard(ref_train.Jaccard):
    made = []

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        RecJaccard.made.append(self)


class RecStat(ref_train.StatManager):
    made = []

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        RecStat.made.append(self)


class NullWriter:
    def add_scalar(self, *a, **k):
        pass


def run_validation(stub, loader, step_func, ignore):
    """One `Trainer.validation` call; returns (score, {layer: Jaccard}, StatManager, [masks per evaluated batch])."""
    RecJaccard.made, RecStat.made = [], []
    seen = []

    def recording_step(*a, **k):
        losses, masks = step_func(*a, **k)
        seen.append({key: val.detach().clone() for key, val in masks.items() if torch.is_tensor(val)})
        return losses, masks
    ref_cfg.VAL.IGNORE_CLASS = list(ignore)
    score = ref_train.Trainer.validation(stub, 0, NullWriter(), loader, tag=None, step_func=recording_step, max_iter=MAX_ITER)
    ref_cfg.VAL.IGNORE_CLASS = []
    layers = [k for k in seen[0] if k in SCORE_LAYERS + (LABEL_LAYER,)]
    assert len(RecJaccard.made) == len(layers) and len(RecStat.made) == 1
    return score, dict(zip(layers, RecJaccard.made)), RecStat.made[0], seen


def counts_of(j):
    return torch.stack([j.tps, j.fps, j.fns]).to(torch.int64).numpy()


def top2_gap(t):
    top = t.topk(2, dim=1).values
    return top[:, 0] - top[:, 1]


def label_margin(probs, chi):
    """min(top-2 gap, |confidence - class threshold|): the thresholds of models/sac.py:159-174 from `teacher_refined`."""
    B, C = probs.shape[:2]
    conf, idx = probs.max(1, keepdim=True)
    peaks = torch.zeros_like(probs).scatter_(1, idx, conf).view(B, C, -1).max(-1).values
    peaks = peaks * ref_cfg.MODEL.RUN_CONF_UPPER * (1. - torch.exp(-chi / ref_cfg.MODEL.THRESHOLD_BETA)).view(1, C)
    peaks = peaks.clamp(ref_cfg.MODEL.RUN_CONF_LOWER)
    thr = peaks.gather(1, idx.view(B, -1)).view(B, *probs.shape[-2:])
    return torch.minimum(top2_gap(probs), (conf[:, 0] - thr).abs())


def store_margin(m, scale):
    return (m / scale).clamp(max=MARGIN_CAP).to(torch.float16).numpy()


def write_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same bytes on every run."""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


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
    ref_train.Jaccard, ref_train.StatManager = RecJaccard, RecStat
    torch.Tensor.cuda = lambda self, *a, **k: self          # train.py:124-125,183 and metrics.py:14-16 on a GPU-less machine

    net = MG.make_sac()
    net.backbone.load_state_dict(nets_ref.resnet101_state(seed=STUDENT_SEED, **STATE_KW), strict=True)
    net.slow_net.load_state_dict(nets_ref.resnet101_state(seed=TEACHER_SEED, **STATE_KW), strict=True)
    net.slow_init[0] = True
    net.eval()
    ref_cfg.TRAIN.NUM_GROUPS, ref_cfg.TRAIN.GROUP_SIZE = N, T
    stub = types.SimpleNamespace(cfg=ref_cfg, net=net, gpu=0, world_size=1, nclass=19, classNames=CLASS_NAMES, main_process=True,
                                 optim=None, visualise_results=lambda *a, **k: None, has_fixed_batch=lambda tag: True)
    stub.step = functools.partial(ref_train.Trainer.step, stub)
    stub._prep_batch = functools.partial(ref_train.Trainer._prep_batch, stub)
    step_source = stub.step
    step_target = functools.partial(ref_train.Trainer._step_target, stub)

    gen = torch.Generator().manual_seed(DATA_SEED)
    aff, inv = view_affines()
    ignore = torch.zeros(N * T, H, W, dtype=torch.bool)    # augmentation padding: the views cover each other's
    ignore[1, :, -2:] = True
    ignore[3, :1] = True
    rec = dict(H=H, W=W, N=N, T=T, BS=BS, max_iter=MAX_ITER, num_batches=NUM_BATCHES, counted=COUNTED, student_seed=STUDENT_SEED,
               teacher_seed=TEACHER_SEED, ignore_synthia=np.array(IGNORE_SYNTHIA), contract=CONTRACT, margin_cap=MARGIN_CAP,
               affine=aff, affine_inv=inv, win=np.array([WIN_ROW0, WIN_ROWS, WIN_VIEWS, WIN_BATCHES]))

    # ---- inputs ---------------------------------------------------------------------------------
    src, tgt = [], []
    with torch.no_grad():
        for b in range(COUNTED):
            xs = blocky(gen, (BS, 3, H, W))
            f2 = blocky(gen, (N * T, 3, H, W))
            f1 = f2 + blocky(gen, (N * T, 3, 1, 1), 1) / 4          # a per-view, per-channel brightness shift
            stu_s = net.backbone(xs)[1].argmax(1)
            tea_s = net.slow_net(xs)[1].argmax(1)
            stu_t = net.backbone(f1)[1].argmax(1)
            tea_logits = net.slow_net(f2)[1]
            if b == 0:                                              # the class prior: what the first update would store
                chi = torch.softmax(tea_logits, 1).mean(0).view(19, -1).mean(-1)
                net.running_conf.copy_(chi)
                rec["running_conf"] = net.running_conf.clone()
            ys = mixed_gt(gen, stu_s, tea_s)
            gt = mixed_gt(gen, tea_logits.argmax(1), stu_t)         # the teacher's share is the larger one: it takes the score
            gt[ignore] = -1                                         # augmentation padding (dataloader_target.py)
            src.append((xs, ys))
            tgt.append((f1, gt, f2))
            rec.update({"src%d_x" % b: xs, "src%d_y" % b: ys.to(torch.int16), "tgt%d_f1" % b: f1, "tgt%d_f2" % b: f2,
                        "tgt%d_gt" % b: gt.to(torch.int16)})
    chi = net.running_conf.clone()

    def source_loader():      # the 4th batch repeats the 1st: if it were counted, the counts would show it
        return [(src[b % COUNTED][0].clone(), src[b % COUNTED][1].clone()) for b in range(NUM_BATCHES)]

    def target_loader():
        out = []
        for b in range(NUM_BATCHES):
            f1, gt, f2 = tgt[b % COUNTED]
            out.append(tuple(t.clone().view(N, T, *t.shape[1:]) for t in (f1, gt, f2, aff, inv)))
        return out

    # ---- the reference's validation, both ignore lists, both passes ----------------------------------
    for name, loader_fn, step_func in (("src", source_loader, step_source), ("tgt", target_loader, step_target)):
        for tag, ignore_list in (("none", []), ("synthia", IGNORE_SYNTHIA)):
            score, jac, stat, seen = run_validation(stub, loader_fn(), step_func, ignore_list)
            assert len(seen) == COUNTED, len(seen)
            rec["%s_score_%s" % (name, tag)] = np.float64(score)
            for layer, j in jac.items():
                ja, pr, re = j.summarise()
                keep = [i for i in range(19) if i not in ignore_list]
                rec["%s_%s_mean_%s" % (name, layer, tag)] = np.array([float(v[keep].mean()) for v in (ja, pr, re)], np.float64)
        rec[name + "_layers"] = np.array(list(jac))
        for key, val in stat.items():
            rec["%s_loss_%s" % (name, key)] = np.float64(val)
        rec[name + "_loss_keys"] = np.array([k for k, _ in stat.items()])
        for layer, j in jac.items():
            ja, pr, re = j.summarise()
            rec["%s_%s_counts" % (name, layer)] = counts_of(j)
            rec["%s_%s_summary" % (name, layer)] = torch.stack([ja, pr, re]).numpy()
        for b, masks in enumerate(seen):
            rec["%s%d_gt_seen" % (name, b)] = masks["mask_gt"].to(torch.uint8)         # after -1 -> 255
            for layer in jac:
                t = masks[layer]
                if layer == LABEL_LAYER:
                    rec["%s%d_%s_map" % (name, b, layer)] = t.to(torch.uint8)
                    rec["%s%d_%s_margin" % (name, b, layer)] = store_margin(label_margin(masks["teacher_refined"], chi),
                                                                            masks["teacher_refined"].abs().max())
                else:
                    rec["%s%d_%s_map" % (name, b, layer)] = t.argmax(1).to(torch.uint8)
                    rec["%s%d_%s_margin" % (name, b, layer)] = store_margin(top2_gap(t), t.abs().max())
        if name == "tgt":
            tgt_seen, tgt_jac = seen, jac

    # ---- full layer tensors on a window, with the reference Jaccard's counts on exactly that window ----------
    rows = slice(WIN_ROW0, WIN_ROW0 + WIN_ROWS)
    win_jac = {layer: ref_train.Jaccard(19, 0) for layer in tgt_jac}
    for b in range(WIN_BATCHES):
        masks = tgt_seen[b]
        gt_w = masks["mask_gt"][:WIN_VIEWS, rows].clone()
        rec["win%d_gt" % b] = gt_w.to(torch.uint8)
        for layer in tgt_jac:
            t = masks[layer][:WIN_VIEWS, ..., rows, :].contiguous()
            rec["win%d_%s" % (b, layer)] = t.to(torch.uint8) if layer == LABEL_LAYER else t
            pred = t.clone() if layer == LABEL_LAYER else torch.argmax(t, 1)
            win_jac[layer].add_sample(pred, gt_w.clone())
        for layer in tgt_jac:
            rec["win%d_%s_counts" % (b, layer)] = counts_of(win_jac[layer])              # accumulated over the windows so far

    # ---- the conditions that keep the tests from passing vacuously ------------------------------------
    labels = np.concatenate([rec["tgt%d_teacher_labels_map" % b].numpy().ravel() for b in range(COUNTED)])
    share = float((labels != 255).mean())
    print("labelled share of teacher_labels: {:.3f}".format(share))
    assert 0.20 <= share <= 0.80, share
    for name in ("src", "tgt"):
        present = set(np.unique(np.concatenate([rec["%s%d_gt_seen" % (name, b)].numpy().ravel() for b in range(COUNTED)]))) - {255}
        print(name, "classes in the ground truth:", len(present))
        assert present == set(range(19)), sorted(present)
        for layer in rec[name + "_layers"]:
            c = rec["%s_%s_counts" % (name, layer)]
            print("  {:16s} tp {:6d} fp {:6d} fn {:6d}  mIoU {:.4f} / {:.4f}".format(
                layer, int(c[0].sum()), int(c[1].sum()), int(c[2].sum()), rec["%s_%s_mean_none" % (name, layer)][0],
                rec["%s_%s_mean_synthia" % (name, layer)][0]))
            assert (c[1] > 0).any() and (c[2] > 0).any(), (name, layer)
            low = np.concatenate([(rec["%s%d_%s_margin" % (name, b, layer)].astype(np.float32) < CONTRACT).ravel() for b in range(COUNTED)])
            print("    pixels with a margin below the contract: {:.4f}".format(float(low.mean())))
            assert low.mean() <= 0.01, (name, layer, float(low.mean()))
        print(name, "score", rec[name + "_score_none"], rec[name + "_score_synthia"], "losses",
              {k: float(rec["%s_loss_%s" % (name, k)]) for k in rec[name + "_loss_keys"]})
    mious = [rec["tgt_%s_mean_none" % layer][0] for layer in rec["tgt_layers"]]
    assert min(abs(mious[0] - m) for m in mious[1:]) > 1e-3, mious          # a "max over layers" that looked at one layer is caught
    for b in range(WIN_BATCHES):
        assert (rec["win%d_gt" % b].numpy() != 255).any()

    out = {}
    for k, v in rec.items():
        out[k] = np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v)
    path = os.path.join(HERE, "g19_validation.npz")
    write_npz(path, out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
