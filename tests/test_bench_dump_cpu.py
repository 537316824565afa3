"""bench.py --dump-outputs on CPU tensors: what a training step returned and the state it left, as .npy files that are the
same from run to run (large arrays as a seeded sample at fixed positions), in float32 / float64, within the size budget."""
import os
import zlib

import numpy as np
import torch
import torch.nn as nn

import bench


def _step_result():
    gen = torch.Generator().manual_seed(0)
    losses_src = {"loss_ce": torch.tensor(1.25)}
    losses_tgt = {"self_ce": torch.tensor([0.5]), "teacher_diff": torch.tensor([0.125], dtype=torch.float64)}
    outs = {"logits_up": torch.randn(2, 3, 40, 50, generator=gen),
            "teacher_labels": torch.randint(0, 19, (2, 40, 50), generator=gen),
            "mask": torch.rand(2, 40, 50, generator=gen) > 0.5,
            "not_a_tensor": 3}
    return losses_src, losses_tgt, outs


def _net():
    torch.manual_seed(0)
    net = nn.Sequential(nn.Conv2d(3, 8, 3), nn.BatchNorm2d(8))
    net[1].num_batches_tracked.fill_(7)          # an integer buffer: not part of `state`
    return net


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_names_dtypes_and_exact_small_arrays(tmp_path):
    res, net = _step_result(), _net()
    bench.dump_outputs(str(tmp_path), res, net)
    got = _load(str(tmp_path))
    assert sorted(got) == ["out_logits_up", "out_mask", "out_teacher_labels", "src_loss_ce", "state", "tgt_self_ce",
                           "tgt_teacher_diff"]
    assert got["src_loss_ce"].dtype == np.float32 and float(got["src_loss_ce"]) == 1.25
    assert got["tgt_teacher_diff"].dtype == np.float64 and got["out_teacher_labels"].dtype == np.float64
    assert got["out_logits_up"].dtype == np.float32 and got["out_mask"].dtype == np.float32
    assert np.array_equal(got["out_logits_up"], res[2]["logits_up"].numpy())
    assert np.array_equal(got["out_teacher_labels"], res[2]["teacher_labels"].numpy())
    state = torch.cat([v.flatten().float() for v in net.state_dict().values() if v.is_floating_point()])
    assert np.array_equal(got["state"], state.numpy())


def test_dump_outputs_samples_large_arrays_at_fixed_positions_within_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 4096)
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 40000)
    res, net = _step_result(), _net()
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), res, net)
    bench.dump_outputs(str(b), _step_result(), _net())
    got, again = _load(str(a)), _load(str(b))
    for k in got:                                  # the same inputs give the same files
        assert np.array_equal(got[k], again[k]), k
    assert sum(os.path.getsize(os.path.join(str(a), f)) - 128 for f in os.listdir(str(a))) <= 40000
    n = got["out_logits_up"].size
    assert n < res[2]["logits_up"].numel() and n == got["out_teacher_labels"].size      # one cap for every large array
    assert got["src_loss_ce"].size == 1
    # a sample of the array itself, at sorted positions drawn from a generator seeded with crc32(name)
    full = res[2]["logits_up"].flatten()
    idx = torch.randint(full.numel(), (n,), generator=torch.Generator().manual_seed(zlib.crc32(b"out_logits_up"))).sort().values
    assert np.array_equal(got["out_logits_up"], full[idx].numpy())
