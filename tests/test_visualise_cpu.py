"""Epoch summary panels, the part that needs no GPU: the g20 fixture is self-consistent and not vacuous, the palette and the
colour map are the reference's, panel bookkeeping, the grid layout, the rank-major gather over gloo, the fixed-batch cache.

EPS = 2e-5 (the upper end of the project's measured kernel-against-oracle deviation) decides which pixels are exempt:
a class-overlay pixel when the reference's top-2 gap of the resized scores is below EPS (stored `gap` < 1), a confidence-overlay
pixel when 256 (1 - conf) is within 256 EPS of an integer (stored `frac` <= 1) or the class pixel of the same read is exempt.  At
most 3 % of any panel may be exempt: a condition on the fixture, asserted here from the stored margins."""
import os

import numpy as np
import pytest
import torch

READS = ("prediction", "teacher_init", "teacher_aligned", "teacher_refined")
PASSES = {"source": 4, "target": 13}


@pytest.fixture(scope="module")
def g20(golden):
    return golden("g20_visualise")


def test_fixture_is_self_consistent_and_within_the_exemption_cap(g20):
    assert float(g20["eps"]) == 2e-5 and float(g20["max_exempt"]) == 0.03
    B = int(g20["B"])
    for run in g20["runs"]:
        h, w = (int(v) for v in g20[run + "_size"])
        y0, y1, x0, x1 = (int(v) for v in g20[run + "_window"])
        assert (h, w) != (y1 - y0, x1 - x0)
        for name, P in PASSES.items():
            strip, rows = g20["%s_%s_strip" % (run, name)], g20["%s_%s_rows" % (run, name)]
            assert strip.shape == (B, 3, h, P * w) and strip.dtype == np.float32 and rows.shape == strip.shape and rows.dtype == np.uint8
            assert np.array_equal(rows, np.clip(strip * np.float32(255), 0, 255).astype(np.uint8))       # base_trainer.py:264
        for read in READS:
            gap, frac = g20["%s_%s_gap" % (run, read)].astype(np.float32), g20["%s_%s_frac" % (run, read)].astype(np.float32)
            assert gap.shape == (B, h, w) and frac.shape == (B, h, w)
            assert float((gap < 1).mean()) <= 0.03, (run, read)
            assert float(((frac <= 1) | (gap < 1)).mean()) <= 0.03, (run, read)
        assert float((g20[run + "_teacher_conf_frac"].astype(np.float32) <= 1).mean()) <= 0.03
    assert g20["shrink_size"][0] < g20["H"] and g20["enlarge_size"][0] > g20["enlarge_window"][1] - g20["enlarge_window"][0]


def test_fixture_is_not_vacuous(g20):
    gt, loaded = g20["masks_gt"], g20["gt_loaded"]
    assert set(np.unique(gt)) >= set(range(19)) | {255}
    assert (loaded == -1).any() and np.array_equal(gt[loaded == -1], np.full(int((loaded == -1).sum()), 255, np.uint8))
    assert np.array_equal(gt[loaded != -1], loaded[loaded != -1].astype(np.uint8))
    share = float((g20["out_teacher_labels"] != 255).mean())
    assert 0.20 <= share <= 0.80, share
    for run in g20["runs"]:
        w = int(g20[run + "_size"][1])
        strip = g20[run + "_target_strip"]
        panel = lambda i: strip[..., i * w:(i + 1) * w]
        init, aligned, refined = panel(7), panel(9), panel(11)
        assert not np.array_equal(init, aligned) and not np.array_equal(aligned, refined) and not np.array_equal(init, refined)
    assert list(g20["source_keys"]) == ["logits", "logits_up"]
    for key in ("logits_up", "teacher_init", "teacher_refined", "teacher_conf", "teacher_labels", "running_conf", "teacher_aligned", "frames_aligned"):
        assert key in list(g20["target_keys"])


def test_palette_is_the_references_and_saturates_like_pillow(g20):
    import visualise as V
    assert V.CS_PALETTE.shape == (256, 3) and V.CS_PALETTE.dtype == np.uint8
    assert np.array_equal(V.CS_PALETTE, g20["palette"])
    assert not V.CS_PALETTE[19:].any()
    labels = g20["saturation_labels"]
    assert {-1, 19, 254, 255, 300} <= set(labels.ravel().tolist())
    idx = V.palette_index(labels)
    assert idx.ravel().tolist()[:5] == [0, 19, 254, 255, 255]
    assert np.array_equal(V.CS_PALETTE[idx.ravel()], g20["saturation_rgb"])


def test_colormap_is_the_references_table(g20):
    import visualise as V
    table = V.colormap("inferno")
    assert table.shape == (256, 3) and table.dtype == np.float32
    assert np.array_equal(table, g20["inferno"].astype(np.float32))
    assert np.array_equal(V.colormap("inferno", table=g20["inferno"]), table)
    with pytest.raises(ValueError):
        V.colormap("inferno", table=np.zeros((255, 3)))
    # index rule: trunc(256 v) in float32, clipped to 0..255
    v = g20["inferno_probe"]
    idx = np.clip((v * np.float32(256)).astype(np.int64), 0, 255)
    assert np.array_equal(g20["inferno"][idx], g20["inferno_probe_rgb"])


def test_panel_names():
    import visualise as V
    assert V.panel_names({"logits_up": 0}) == ["image", "ground_truth", "prediction", "confidence"]
    full = dict.fromkeys(["logits_up", "teacher_init", "teacher_refined", "teacher_conf", "teacher_labels", "running_conf", "teacher_aligned",
                          "frames_aligned"])
    assert V.panel_names(full, image2=1) == list(V.PANELS) and len(V.PANELS) == 13
    assert V.panel_names({"logits_up": 0, "teacher_labels": 0}, image2=1) == ["image", "ground_truth", "teacher_labels", "prediction",
                                                                            "confidence", "image2"]
    assert V.panel_names({"logits_up": 0, "teacher_conf": 0, "teacher_refined": 0}) == [
        "image", "ground_truth", "prediction", "confidence", "teacher_conf", "teacher_refined", "teacher_refined_conf"]


def host_grid(rows, padding=8, pad=229):
    """The layout the issue defines: [3, B (h+8) + 8, W + 8] filled with 229, row k at y = k (h+8) + 8, x = 8; one row unpadded."""
    B, _, h, w = rows.shape
    if B == 1:
        return rows[0].copy()
    out = np.full((3, B * (h + padding) + padding, w + padding), pad, np.uint8)
    for k in range(B):
        out[:, k * (h + padding) + padding:k * (h + padding) + padding + h, padding:padding + w] = rows[k]
    return out


@pytest.mark.parametrize("B,h,w", [(1, 5, 12), (2, 5, 12), (3, 1, 7)])
def test_to_grid_layout(B, h, w):
    import visualise as V
    rows = torch.randint(0, 256, (B, 3, h, w), dtype=torch.uint8, generator=torch.Generator().manual_seed(B))
    grid = V.to_grid(rows)
    assert grid.dtype == torch.uint8 and tuple(grid.shape) == V.grid_shape(B, h, w)
    assert np.array_equal(grid.numpy(), host_grid(rows.numpy()))
    if B > 1:
        assert int(grid[0, 0, 0]) == int(0.9 * 255) == 229 and tuple(grid.shape) == (3, B * (h + 8) + 8, w + 8)


def test_ops_and_float_grid_refuse_cpu_tensors():
    import visualise as V
    from dasac_hip import ops, DasacError
    image = torch.zeros(1, 3, 4, 4)
    with pytest.raises(DasacError):
        ops.vis_panels([(ops.VIS_IMAGE, image, None, False, 0, 0)], (2, 2), 1, V.MEAN, V.STD, torch.zeros(256, 3, dtype=torch.uint8),
                       torch.zeros(256, 3))
    with pytest.raises(DasacError):
        ops.vis_grid(torch.zeros(2, 3, 4, 4))
    with pytest.raises(DasacError):
        V.to_grid(torch.zeros(2, 3, 4, 4))
    with pytest.raises(DasacError):
        V.render(image, torch.zeros(1, 4, 4, dtype=torch.int64), {"logits_up": torch.zeros(1, 19, 4, 4)}, im_size=(2, 2))


def test_driver_exports():
    import driver
    assert callable(driver.visualise_results)
    cache = driver.FixedBatches()
    assert not cache.has_fixed_batch("train")
    x, y = torch.arange(6.).view(1, 6), torch.arange(3)
    cache.save_fixed_batch("train", (x, y, "name"))
    assert cache.has_fixed_batch("train") and not cache.has_fixed_batch("train_target")
    kept = cache["train"]
    x += 1                                                   # host CLONES: the cache does not follow the caller's tensors
    assert torch.equal(kept[0], torch.arange(6.).view(1, 6)) and torch.equal(kept[1], y) and kept[2] == "name"
    assert kept[0].device.type == "cpu"
    cache.save_fixed_batch("train", (x,))                    # updating a tag replaces it
    assert len(cache["train"]) == 1 and torch.equal(cache["train"][0], x)


def _gather_rank(rank, world, port, q):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "da-sac_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import visualise as V
    rows = torch.full((2, 3, 4, 5), 10 * rank, dtype=torch.uint8) + torch.arange(2, dtype=torch.uint8).view(2, 1, 1, 1)
    conf = torch.arange(19, dtype=torch.float32) + 100 * rank
    got, confs = V.gather_rows(rows, conf)
    q.put((rank, got.numpy(), confs))
    dist.barrier()
    dist.destroy_process_group()


def test_gather_rows_is_rank_major_over_gloo():
    import queue
    import socket
    import torch.multiprocessing as mp
    import visualise as V
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gather_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        got = sorted((q.get(timeout=120) for _ in procs), key=lambda t: t[0])
    except queue.Empty:
        got = None
    for p in procs:
        p.join(30)
        if p.is_alive():
            p.kill()
    assert got is not None and [p.exitcode for p in procs] == [0, 0]
    for rank, rows, confs in got:
        assert rows.shape == (4, 3, 4, 5)
        assert [int(rows[i, 0, 0, 0]) for i in range(4)] == [0, 1, 10, 11]                     # rank-major along the batch
        assert confs == pytest.approx([c + 50.0 for c in range(19)])                           # view(-1, C).mean(0)
    # no process group: the rows as they are, the prior's own values
    rows, confs = V.gather_rows(torch.zeros(1, 3, 2, 2, dtype=torch.uint8), torch.arange(19.))
    assert rows.shape == (1, 3, 2, 2) and confs == list(range(19))
    assert V.gather_rows(rows)[1] is None
