"""driver.py / reports.py after the split (CPU): reports.py stands alone and driver re-exports it, the eval-mode guard restores
the mode when its body raises, and the rank-sum helper sums on the host under gloo."""
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "da-sac_amd")
MOVED = ("summarise_iou counts_from_confusion summarise_confusion pseudo_label_audit summarise_reliability format_confusion "
         "summarise_boundary format_boundary summarise_consistency format_consistency gradient_report skipped_step_report "
         "format_gradient_report activation_report moment_gap domain_gap_report format_activation_report format_domain_gap_report "
         "class_gap_report format_class_gap_report stat_mean class_subset_mean summarise_validation").split()


def test_reports_imports_without_the_driver_or_the_kernels():
    code = ("import sys; sys.path.insert(0, {!r}); import reports; "
            "bad = [m for m in sys.modules if m.split('.')[0] in ('driver', 'dasac_hip', 'visualise')]; assert not bad, bad").format(PKG)
    subprocess.run([sys.executable, "-c", code], check=True, timeout=120)


def test_driver_re_exports_every_reader():
    import driver
    import reports
    public = [n for n, v in vars(reports).items() if not n.startswith("_") and getattr(v, "__module__", None) == "reports"]
    assert sorted(public) == sorted(MOVED)
    for name in MOVED:
        assert getattr(driver, name) is getattr(reports, name), name
    assert driver.FixedBatches is not None and callable(driver._ms_plan) and callable(driver._dist_state)


@pytest.mark.parametrize("training", [True, False])
def test_eval_mode_restores_the_mode_when_the_body_raises(training):
    import driver
    net = torch.nn.Sequential(torch.nn.Linear(2, 2), torch.nn.BatchNorm1d(2)).train(training)
    with pytest.raises(RuntimeError, match="inside"):
        with driver.eval_mode(net) as inside:
            assert inside is net and not net.training and not net[1].training
            raise RuntimeError("inside")
    assert net.training is training and net[1].training is training
    with driver.eval_mode(net):
        assert not net.training
    assert net.training is training


def _rank_sum_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, PKG)
    import driver
    mine = torch.arange(6, dtype=torch.int64).view(2, 3) * (rank + 1) + 100 * rank
    got = driver.rank_sum(mine)
    q.put((rank, got.device.type, str(got.dtype), got.tolist()))
    dist.barrier()
    dist.destroy_process_group()


def test_rank_sum_across_two_ranks_gloo():
    import driver
    alone = torch.arange(6, dtype=torch.int64).view(2, 3)
    assert driver.rank_sum(alone) is alone and torch.equal(alone, torch.arange(6).view(2, 3))      # no process group: untouched
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = [ctx.Process(target=_rank_sum_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    want = (torch.arange(6).view(2, 3) * 3 + 100).tolist()
    assert res == [(0, "cpu", "torch.int64", want), (1, "cpu", "torch.int64", want)]
