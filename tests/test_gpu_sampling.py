"""dasac_label_hist (csrc/sampling.hip) and driver.compute_sample_weights on the MI355X.  Every call goes through the C ABI;
the oracle is np.bincount(minlength=256) per image and equality is exact (integer counts)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

HWS = [1, 15, 16, 17, 63, 64, 65, 4095, 4097, 769 * 769, 1024 * 2048]
BS = [1, 3, 8]


def bincount(maps):
    """[B,256] int64 of a host uint8 array [B, ...]"""
    maps = np.asarray(maps)
    return np.stack([np.bincount(m.ravel(), minlength=256) for m in maps.reshape(maps.shape[0], -1)]).astype(np.int64)


def g18_maps(g):
    return [g["labels%d" % n] for n in range(len(g["names"]))]


def blocky(g, B, H, W):
    """realistic label maps: the g18 maps, nearest-upsampled to H x W"""
    out = np.empty((B, H, W), np.uint8)
    maps = g18_maps(g)
    for b in range(B):
        m = maps[(b * 5 + 1) % len(maps)]
        out[b] = m[(np.arange(H) * m.shape[0] // H)[:, None], (np.arange(W) * m.shape[1] // W)[None, :]]
    return out


def content(kind, B, HW, g, seed=0):
    rng = np.random.RandomState(seed)
    if kind == "uniform":
        return rng.randint(0, 256, size=(B, HW)).astype(np.uint8)
    if kind.startswith("const"):
        return np.full((B, HW), int(kind[5:]), np.uint8)
    if kind == "stripes":                                   # 64-pixel stripes, phase shifted per image
        return (((np.arange(HW)[None, :] + 7 * np.arange(B)[:, None]) // 64) % 19).astype(np.uint8)
    assert kind == "blocky"
    W = max(1, int(np.sqrt(2 * HW)))
    H = (HW + W - 1) // W
    return blocky(g, B, H, W).reshape(B, -1)[:, :HW].copy()


def run(host):
    """host uint8 [B,HW] -> int64 [B,256] through ops.label_hist on a [B,1,HW] device tensor"""
    from dasac_hip import ops
    dev = torch.from_numpy(np.ascontiguousarray(host)).cuda()
    return ops.label_hist(dev.view(dev.shape[0], 1, -1)).cpu().numpy()


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("HW", HWS)
def test_label_hist_sizes_uniform_labels(HW, B, golden):
    host = content("uniform", B, HW, None, seed=HW % 1000 + B)
    got = run(host)
    assert got.dtype == np.int64 and got.shape == (B, 256)
    assert np.array_equal(got, bincount(host))
    assert (got.sum(1) == HW).all()


@pytest.mark.parametrize("kind", ["const0", "const18", "const255", "stripes", "blocky"])
@pytest.mark.parametrize("HW,B", [(17, 3), (65, 8), (4097, 3), (769 * 769, 3), (1024 * 2048, 8)])
def test_label_hist_run_contents(kind, HW, B, golden):
    host = content(kind, B, HW, golden("g18_is_sampling"))
    got = run(host)
    assert np.array_equal(got, bincount(host))
    assert (got.sum(1) == HW).all()


def test_label_hist_blocky_images_hw_layout(golden):
    from dasac_hip import ops
    host = blocky(golden("g18_is_sampling"), 4, 512, 1024)
    dev = torch.from_numpy(host).cuda()
    assert np.array_equal(ops.label_hist(dev).cpu().numpy(), bincount(host))
    assert np.array_equal(ops.label_hist(dev[2]).cpu().numpy(), bincount(host[2:3]))          # [H,W]


@pytest.mark.parametrize("offset", range(1, 16))
def test_label_hist_unaligned_views(offset):
    from dasac_hip import ops
    rng = np.random.RandomState(offset)
    B, H, W = 3, 37, 61                                      # odd HW: every image starts at another alignment
    flat = rng.randint(0, 256, size=B * H * W + 64).astype(np.uint8)
    flat[offset + 100:offset + 1500] = 7                     # a run, so that the merged paths are on unaligned data too
    buf = torch.from_numpy(flat).cuda()
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + B * H * W].view(B, H, W)
    assert view.data_ptr() % 16 == offset and view.is_contiguous()
    got = ops.label_hist(view).cpu().numpy()
    assert np.array_equal(got, bincount(flat[offset:offset + B * H * W].reshape(B, -1)))


def test_label_hist_accumulates_and_repeats_bit_equal(golden):
    from dasac_hip import ops
    host = np.concatenate([content("uniform", 2, 769 * 769, None, 3), content("blocky", 2, 769 * 769, golden("g18_is_sampling"))])
    dev = torch.from_numpy(host).cuda().view(4, 769, 769)
    start = torch.arange(4 * 256, dtype=torch.int64).view(4, 256) * 1000003 + (1 << 40)
    counts = start.clone().cuda()
    out = ops.label_hist(dev, counts)
    assert out.data_ptr() == counts.data_ptr()
    assert np.array_equal(counts.cpu().numpy(), start.numpy() + bincount(host))
    ops.label_hist(dev, counts)
    assert np.array_equal(counts.cpu().numpy(), start.numpy() + 2 * bincount(host))
    a, b = ops.label_hist(dev), ops.label_hist(dev)
    assert torch.equal(a, b)


def test_label_hist_more_than_2_to_32_pixels_in_one_call():
    from dasac_hip import ops
    B, H, W = 2049, 1024, 2048                               # B*HW = 2^32 + 2^21
    need = B * H * W + (64 << 20)
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip("needs {:.1f} GiB of free device memory, {:.1f} GiB are free".format(need / 2 ** 30, free / 2 ** 30))
    dev = torch.full((B, H, W), 11, dtype=torch.uint8, device="cuda")
    dev[-1, -1, -3:] = 200                                   # the far end of the buffer is read, and as image B-1
    dev[1024, 0, 0] = 3                                      # around the 2^31 byte mark
    got = ops.label_hist(dev).cpu().numpy()
    del dev
    want = np.zeros((B, 256), np.int64)
    want[:, 11] = H * W
    want[-1, 11] -= 3
    want[-1, 200] = 3
    want[1024, 11] -= 1
    want[1024, 3] = 1
    assert np.array_equal(got, want)


def test_label_hist_rejects_bad_arguments_on_the_host():
    from dasac_hip import lib as L
    lib = L.load()
    x = torch.zeros(64, dtype=torch.uint8, device="cuda")
    counts = torch.zeros((1, 256), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    EINVAL = -1
    s = L.stream_ptr()
    assert lib.dasac_label_hist(x.data_ptr(), 0, 64, counts.data_ptr(), s) == EINVAL
    assert lib.dasac_label_hist(x.data_ptr(), -1, 64, counts.data_ptr(), s) == EINVAL
    assert lib.dasac_label_hist(x.data_ptr(), 1, 0, counts.data_ptr(), s) == EINVAL
    assert lib.dasac_label_hist(None, 1, 64, counts.data_ptr(), s) == EINVAL
    assert lib.dasac_label_hist(x.data_ptr(), 1, 64, None, s) == EINVAL
    assert b"label_hist" in lib.dasac_last_error()
    torch.cuda.synchronize()
    assert int(counts.sum()) == 0                            # nothing was launched
    from dasac_hip import ops
    with pytest.raises(L.DasacError):
        ops.label_hist(x.view(8, 8).long())
    with pytest.raises(L.DasacError):
        ops.label_hist(x.view(8, 8).t())
    with pytest.raises(L.DasacError):
        ops.label_hist(x.view(8, 8).cpu())


def test_g18_end_to_end_weights_bit_equal(golden):
    """maps -> device -> label_hist -> weights_from_counts == the reference tool's weights, bit for bit; images of different
    sizes go in separate launches into the rows of one table."""
    import sampling
    from dasac_hip import ops
    g = golden("g18_is_sampling")
    names = [str(n) for n in g["names"]]
    table = torch.zeros((len(names), 256), dtype=torch.int64, device="cuda")
    for n, m in enumerate(g18_maps(g)):
        ops.label_hist(torch.from_numpy(m).cuda(), table[n:n + 1])
    w = sampling.weights_from_counts(names, table)
    for n, name in enumerate(names):
        want = {int(v): float(g["weights"][n, v]) for v in np.flatnonzero(g["present"][n])}
        assert w[name] == want, name
    index = {n: i for i, n in enumerate(names)}
    tables = sampling.init_sampling(len(names), w, index, 19, [], float(g["prior_weight"]))
    assert np.array_equal(np.array(tables), g["tables_none"])


# ------------------------------------------------------------------------------------------------
# driver.compute_sample_weights
# ------------------------------------------------------------------------------------------------
N_IMAGES, SIZE = 5, (65, 97)


def _net(arch):
    import torch.nn as nn
    sys.path.insert(0, ROOT)
    import bench
    import driver
    import models
    cfg = bench.model_cfg(arch)
    net = models.get_model(cfg, 0, num_classes=19, criterion=nn.CrossEntropyLoss(ignore_index=255, reduction="none"))
    driver.init_synthetic_weights(net, seed=1)
    return net.cuda().eval()


def _images():
    g = torch.Generator().manual_seed(5)
    return torch.randn(N_IMAGES, 3, *SIZE, generator=g)


def _batches(images, index_lists):
    for idx in index_lists:
        yield images[idx].cuda(), idx


@pytest.mark.parametrize("arch", ["deeplabv2_resnet101", "fcn_vgg16_bn"])
def test_compute_sample_weights_equals_bincount_of_the_label_maps(arch):
    import driver
    net = _net(arch)
    images = _images()
    splits = [[0, 1], [2, 3], [4]]
    for lut in (None, driver.CITYSCAPES_TRAIN_TO_ID):
        table = driver.compute_sample_weights(net, _batches(images, splits), N_IMAGES, lut=lut)
        assert not table.is_cuda and table.dtype == torch.int64 and tuple(table.shape) == (N_IMAGES, 256)
        maps = torch.cat([driver.infer_label_maps(net, x, lut=lut)[0].cpu() for x, _ in _batches(images, splits)])
        assert np.array_equal(table.numpy(), bincount(maps.numpy()))
        assert (table.sum(1) == SIZE[0] * SIZE[1]).all()
        allowed = set(range(19)) if lut is None else set(driver.CITYSCAPES_TRAIN_TO_ID)
        assert set(np.flatnonzero(table.sum(0).numpy()).tolist()) <= allowed
        assert len(np.flatnonzero(table.sum(0).numpy())) > 1
    assert not net.training
    # rows no batch touches stay zero; scattered indices land in their own rows
    part = driver.compute_sample_weights(net, _batches(images, [[4, 1]]), N_IMAGES)
    maps = driver.infer_label_maps(net, images[[4, 1]].cuda())[0].cpu().numpy()
    assert np.array_equal(part[[4, 1]].numpy(), bincount(maps)) and int(part[[0, 2, 3]].sum()) == 0


RANK_BATCHES = ([[0, 2], [4]], [[1, 3]])                   # images 0::2 and 1::2


def _rank_main(rank, port, queue):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        for p in (ROOT, os.path.join(ROOT, "da-sac_amd"), os.path.join(ROOT, "tests")):
            if p not in sys.path:
                sys.path.insert(0, p)
        from conftest import init_ranks
        import torch.distributed as dist
        import driver
        init_ranks(rank, 2)
        net = _net("deeplabv2_resnet101")
        images = _images()
        assert sorted(sum(RANK_BATCHES[rank], [])) == list(range(N_IMAGES))[rank::2]
        table = driver.compute_sample_weights(net, _batches(_images(), RANK_BATCHES[rank]), N_IMAGES)
        queue.put((rank, table.numpy()))
        dist.barrier()
        dist.destroy_process_group()
    except BaseException as exc:          # the parent reports it; a silent rank would cost the whole timeout
        import traceback
        queue.put((rank, "".join(traceback.format_exception(type(exc), exc, exc.__traceback__))))
        raise


def test_compute_sample_weights_two_ranks_sum_to_the_single_process_table():
    import driver
    from conftest import run_ranks
    got = run_ranks(_rank_main, 2, lambda r, port, q: (r, port, q), timeout=300)
    for r, t in got:
        assert not isinstance(t, str), "rank {} failed:\n{}".format(r, t)
    net = _net("deeplabv2_resnet101")
    # the single process sees the same batches (an image's label map may depend on its batch in the last bits of a logit)
    single = driver.compute_sample_weights(net, _batches(_images(), RANK_BATCHES[0] + RANK_BATCHES[1]), N_IMAGES).numpy()
    assert (single.sum(1) == SIZE[0] * SIZE[1]).all()
    for r, t in got:
        assert np.array_equal(t, single), "rank {}".format(r)
