"""View-sharded target pass (cfg-5's regime): N*L/world < L, so the L views of ONE target image are spread over
consecutive ranks.  2 or 4 ranks (all on the box's one GPU over gloo, or one GPU each over RCCL when the box has them;
DistributedDataParallel on top of the fused engine) run the product's `driver.prep_batch` (train.py:157-209) + the sharded
`_refine` branch (sac.py:198-216, 244-246) inside two full training iterations; every rank's pseudo labels / refined
probabilities / losses / updated parameters are compared with the CPU oracle emulating the same ranks
(oracle.step_ref.ThreadWorld: DDP buffer broadcast before each forward -- quirk 5 --, gradient averaging after each
backward, the two all_gathers).  The fcn_vgg16_bn world-4 case has cfg-5's 8-GPU layout in small: N = 2 target images,
L = 2 views, ONE view per rank -- ranks 0-1 share the image loaded by rank 0, ranks 2-3 the one loaded by rank 1
(train.py:199-209), both all_gathers run, `teacher_aligned` is sliced at `(rank * B) % T` -- so that index math for
rank >= 2 has executed on a device before the first real multi-GPU run.  Worlds stay at 4 or less: the ranks share the
box's one device with the pytest process (conftest.MAX_RANKS_ON_ONE_DEVICE)."""
import os
import socket
from types import SimpleNamespace as NS

import pytest
import torch
import torch.distributed as dist
import torch.nn as nn

from oracle import nets_ref as N
from oracle import step_ref as S
from conftest import rel_err

pytestmark = pytest.mark.gpu

ARCHS = {
    # name -> (state-dict maker, crop (H, W), probe keys)
    "deeplabv2_resnet101": (lambda: N.resnet101_state(seed=3, randomize_bn=True, he_init=True, residual_gain=0.25, aspp_gain=0.2),
                            (33, 49), ("model.conv1.weight", "model.layer3.5.conv2.weight", "model.layer5.conv2d_list.1.bias")),
    "fcn_vgg16_bn": (lambda: _fcn_state(), (64, 96), ("block1.0.weight", "vgg_head.4.bias", "vgg_head.8.bias", "score_pool3.weight")),
}
# Bound on |param - oracle| / max|oracle| after the two iterations.  2e-4 everywhere except `vgg_head.4.bias`: that bias starts at zero
# (after two steps max|param| = 3.5e-4: the comparison IS a gradient comparison) and its gradient is a sum over the 2 x 3 pixels of a
# 64 x 96 crop BEHIND a ReLU of 4096 channels -- one unit whose pre-activation is within fp32 rounding of zero on one side and not on
# the other moves it.  With 8 ranks x 3 crops x 2 passes x 2 iterations 2.4 M such units exist and ~2 of them are borderline at 1e-6
# (measured: 2.9e-3 of max on all ranks alike, deterministic; the oracle in fp32 and in fp64 agree to 4e-7 on this tensor, so the
# oracle side has no flip).  The effect and its fp64 arbitration: tests/test_gpu_models.py::test_resnet101_gradients_fp64_arbitration.
# `vgg_head.8.bias` (the classifier's bias, also zero at the start: a gradient comparison, downstream of the same units) gets the
# contract's 1e-3 (measured 2.2e-4 at 8 ranks); parameters that start at their trained-scale values keep 2e-4.
PARAM_TOL = {"vgg_head.4.bias": 2e-2, "vgg_head.8.bias": 1e-3}
SRC_B, ITERS = 2, 2
# (arch, world, N target images, L views per image): per = N*L/world views per rank < L in every case
CASES = [("deeplabv2_resnet101", 2, 1, 2), ("fcn_vgg16_bn", 2, 1, 2), ("deeplabv2_resnet101", 4, 1, 4), ("fcn_vgg16_bn", 4, 2, 2)]
# (ResNet-101 with one view per rank over two images -- the layout that exposed the gloo point-to-point defect in round 6 at world 8 --
# is left out of the default list only for the suite's time budget; DASAC_TEST_ALL_WORLDS=1 adds it back)
if os.environ.get("DASAC_TEST_ALL_WORLDS") == "1":
    CASES.append(("deeplabv2_resnet101", 4, 2, 2))


def _fcn_state():
    sd = N.fcn8s_vgg16_state(seed=12, randomize_bn=True)
    for k in ("vgg_head.8.weight", "score_pool4.weight", "score_pool3.weight"):      # peaked softmax: thresholds fire
        sd[k] = sd[k] * 2.5
    return sd


def _cfg(arch):
    if arch.startswith("fcn"):                             # configs/fcn_vgg16_train.yaml: LR 5e-4, LR_TARGET 2
        return dict(S.DEFAULT_CFG, ARCH=arch, LR=5e-4, LR_TARGET=2.0)
    return dict(S.DEFAULT_CFG, ARCH=arch)


def _batches(rank, it, hw, world, groups, views):
    """What rank `rank`'s two loaders deliver at iteration `it`: a source batch and max(1, N // world) target images with
    their L views each ([B, L, ...] per tensor, datasets/__init__.py:64-66)."""
    import driver
    loaded_b = max(1, groups // world)
    src, tgt = driver.synthetic_batches(SRC_B, loaded_b, views, hw, "cpu", seed=100 * it + 10 + rank)
    loaded = tuple(t.view((loaded_b, views) + tuple(t.shape[1:])) for t in tgt)
    return src, loaded


def _rank_main(rank, port, case, q):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "da-sac_amd"), os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from conftest import init_ranks
    arch, WORLD, GROUPS, VIEWS = case
    dev = init_ranks(rank, WORLD)
    import driver
    import models
    make_sd, hw, probe = ARCHS[arch]
    cfg = NS(**dict(_cfg(arch), INIT_MODEL="", OPT_NESTEROV=False))
    kw = dict(drop_rate=0.0) if arch.startswith("fcn") else {}           # Dropout p = 0 for parity runs
    net = models.get_model(cfg, rank, num_classes=19, criterion=nn.CrossEntropyLoss(ignore_index=255, reduction="none"), **kw)
    net.backbone.load_state_dict(make_sd(), strict=True)
    net.cuda().train()
    optim = driver.make_optimizer(net, cfg)
    ddp = nn.parallel.DistributedDataParallel(net, device_ids=[dev])
    rec = []
    for it in range(ITERS):
        src, loaded = _batches(rank, it, hw, WORLD, GROUPS, VIEWS)
        src = tuple(t.cuda() for t in src)
        tgt = tuple(driver.prep_batch(t, GROUPS, VIEWS, device="cuda", exchange="p2p" if it else "all_gather") for t in loaded)
        assert tgt[0].shape[0] == GROUPS * VIEWS // WORLD
        assert net.rank == rank and net.world_size == WORLD
        ls, lt, outs = driver.sac_train_iteration(ddp, optim, src, tgt, VIEWS, it == 0, cfg.LR_TARGET)
        logged = driver.reduce_losses(dict(lt))
        rec.append(dict(loss_ce=float(ls["loss_ce"]), self_ce=float(lt["self_ce"]), teacher_diff=float(lt["teacher_diff"]),
                        tgt_loss_ce=float(lt["loss_ce"]), logged=logged, labels=outs["teacher_labels"].cpu().numpy(), refined=outs["teacher_refined"].cpu().numpy(),
                        aligned=outs["teacher_aligned"].cpu().numpy(), chi=net.running_conf.cpu().numpy()))
    torch.cuda.synchronize()
    sd = net.backbone.state_dict()
    q.put((rank, rec, {k: sd[k].detach().cpu().numpy() for k in probe}))
    dist.barrier()
    dist.destroy_process_group()


def _oracle(case):
    arch, WORLD, GROUPS, VIEWS = case
    make_sd, hw, probe = ARCHS[arch]
    tw = S.ThreadWorld(WORLD)

    def rank_fn(r):
        model = S.SacOracle(make_sd(), cfg=_cfg(arch), gather=tw.gather_views(r))
        optim = S.SgdOracle(model)
        rec = []
        for it in range(ITERS):
            src, loaded = _batches(r, it, hw, WORLD, GROUPS, VIEWS)
            ls, lt, outs = S.sharded_sac_iteration(tw, r, model, optim, src, loaded, GROUPS, VIEWS, it == 0)
            rec.append(dict(loss_ce=ls["loss_ce"], self_ce=lt["self_ce"], teacher_diff=lt["teacher_diff"],
                            labels=outs["teacher_labels"], refined=outs["teacher_refined"], aligned=outs["teacher_aligned"],
                            chi=model.running_conf.clone()))
        return rec, {k: model.student[k].detach() for k in probe}
    torch.set_num_threads(max(1, (os.cpu_count() or 2) // WORLD))
    return tw.run(rank_fn)


@pytest.mark.parametrize("case", CASES, ids=["{}-world{}-N{}-L{}".format(*c) for c in CASES])
def test_view_sharded_sac_iterations_vs_oracle(case):
    import threading
    from conftest import run_ranks
    arch, WORLD, GROUPS, VIEWS = case
    ref = {}
    th = threading.Thread(target=lambda: ref.update(out=_oracle(case)))       # the CPU oracle runs while the GPU ranks do
    th.start()
    got = run_ranks(_rank_main, WORLD, lambda r, port, q: (r, port, case, q), timeout=300)
    th.join()
    ref = ref["out"]
    bad = _compare(got, ref, WORLD, GROUPS, VIEWS)
    assert not bad, "\n".join(str(x) for x in bad)


def _compare(got, ref, WORLD, GROUPS, VIEWS):
    """Every violated bound of every (rank, iteration): a failure shows the whole picture, not the first symptom."""
    fired = 0
    bad = []

    def check(ok, *what):
        if not ok:
            bad.append(what)

    close = lambda x, y, rel, abs_=0.0: abs(x - y) <= max(rel * abs(y), abs_)
    for r in range(WORLD):
        rec_r, params_r = ref[r]
        for it in range(ITERS):
            a, b = got[r][1][it], rec_r[it]
            # inputs of the loss first (class prior, aligned and fused probabilities, labels), then the losses built on them
            check(rel_err(a["chi"], b["chi"]) < 1e-4, r, it, "chi", rel_err(a["chi"], b["chi"]))
            check(rel_err(a["aligned"], b["aligned"]) < 1e-4, r, it, "aligned", rel_err(a["aligned"], b["aligned"]))
            check(rel_err(a["refined"], b["refined"]) < 1e-4, r, it, "refined", rel_err(a["refined"], b["refined"]))
            lab = torch.from_numpy(a["labels"])
            assert lab.shape == b["labels"].shape and lab.shape[0] == GROUPS * VIEWS // WORLD
            mism = float((lab != b["labels"]).float().mean())
            check(mism < 1e-3, r, it, "labels", mism, int((lab != 255).sum()), int((b["labels"] != 255).sum()))
            fired += int((lab != 255).sum())
            check(close(a["loss_ce"], b["loss_ce"], 1e-4), r, it, "loss_ce", a["loss_ce"], b["loss_ce"])
            check(close(a["teacher_diff"], b["teacher_diff"], 2e-3, 1e-6), r, it, "teacher_diff", a["teacher_diff"], b["teacher_diff"])
            check(close(a["self_ce"], b["self_ce"], 5e-3, 1e-6), r, it, "self_ce", a["self_ce"], b["self_ce"])
            # train.py:243-246: the logged value is the mean over ranks
            for k in ("self_ce", "teacher_diff", "tgt_loss_ce"):
                mean_k = sum(got[w][1][it][k] for w in range(WORLD)) / WORLD
                check(close(a["logged"][k.replace("tgt_", "")], mean_k, 1e-5, 1e-7), r, it, "logged " + k)
        for k, v in params_r.items():
            check(rel_err(got[r][2][k], v) < PARAM_TOL.get(k, 2e-4), r, "param", k, rel_err(got[r][2][k], v))
    check(fired > 0, "no pseudo label fired: the test would not exercise the loss path")
    # quirk 5: after the last forward the ranks hold different chi (local prior updates); identical parameters though
    for k in got[0][2]:
        for r in range(1, WORLD):
            check(bool((got[0][2][k] == got[r][2][k]).all()), r, "rank-0 parameters", k)
    return bad
