"""The numpy model of the segment ops (tests/segments_ref.py) against scipy.ndimage.label, its tables against mask_counts' counts,
the bin rule, the host-side readers of the tables (reports.summarise_segments / format_segments) and the defaults of the new
arguments.  No GPU."""
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import boundary_ref as BR
import segments_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _maps():
    """Seeded random maps of 2, 3 and 19 classes at blocky scales 1, 3 and 8 with 255 over a tenth of the pixels, and the patterns."""
    rng = np.random.default_rng(7)
    H, W = 37, 53
    out = [(C, SR.random_map(H, W, C, scale, rng)) for C in (2, 3, 19) for scale in (1, 3, 8)]
    out += [(3, f(H, W)) for f in (SR.uniform, SR.checkerboard, SR.diagonals, SR.serpentine, SR.spiral, SR.rings, SR.comb, SR.row_wrap)]
    return out


@pytest.mark.parametrize("connectivity", [4, 8])
def test_the_model_is_scipy_label_per_class_with_smallest_index_roots(connectivity):
    ndimage = pytest.importorskip("scipy.ndimage")
    structure = ndimage.generate_binary_structure(2, 1 if connectivity == 4 else 2)
    for C, m in _maps():
        root, size = SR.segments(m[None], C, connectivity)
        H, W = m.shape
        want_root, want_size = np.full((H, W), -1, np.int32), np.zeros((H, W), np.int32)
        index = np.arange(H * W).reshape(H, W)
        for c in range(C):
            lab, n = ndimage.label(m == c, structure)
            if n:
                smallest = ndimage.minimum(index, lab, np.arange(1, n + 1)).astype(np.int32)
                count = np.bincount(lab.ravel())[1:].astype(np.int32)
                inside = lab > 0
                want_root[inside], want_size[inside] = smallest[lab[inside] - 1], count[lab[inside] - 1]
        assert np.array_equal(root[0], want_root) and np.array_equal(size[0], want_size)
        assert root.dtype == np.int32 and size.dtype == np.int32


def test_patterns_have_the_segments_their_names_promise():
    H, W = 13, 18
    assert len(np.unique(SR.segments(SR.checkerboard(H, W)[None], 2, 4)[0])) == H * W
    assert len(np.unique(SR.segments(SR.checkerboard(H, W)[None], 2, 8)[0])) == 2
    s = SR.serpentine(H, W)
    root, size = SR.segments(s[None], 2, 4)
    assert set(np.unique(root[0][s == 1])) == {0} and int(size[0, 0, 0]) == int((s == 1).sum())
    d = SR.diagonals(H, W)
    assert int(SR.segments(d[None], 3, 4)[1][0][d == 2].max()) == 1 and int(SR.segments(d[None], 3, 8)[1][0][d == 2].max()) > 1
    c = SR.comb(H, W)
    assert set(np.unique(SR.segments(c[None], 2, 4)[0][0][c == 1])) == {0}
    w = SR.row_wrap(H, W)
    both = np.stack([w, w])
    root, size = SR.segments(both, 2, 8)
    assert int(size[0, 2, W - 1]) == 1 and int(size[0, 3, 0]) == 1            # the run ends of two rows stay apart
    assert int(size[0, H - 1, 0]) == W and int(size[1, 0, 0]) == W            # and so do two images
    assert np.array_equal(SR.filter_small(w[None], 2, 2, 255, 8)[0] == 255, (w == 1) & (size[0] == 1))


@pytest.mark.parametrize("connectivity", [4, 8])
def test_tables_summed_over_the_bins_are_the_mask_counts(connectivity):
    rng = np.random.default_rng(11)
    B, C, H, W = 2, 5, 23, 31
    gt = np.stack([SR.random_map(H, W, C, 3, rng) for _ in range(B)])
    gt[0, :4, :4] = -1
    pred = np.stack([SR.random_map(H, W, C, 2, rng) for _ in range(B)])
    hit = rng.random(pred.shape) < 0.5
    pred[hit] = gt[hit]                                                         # half right, 255 and -1 included
    for ignore in (255, 3):
        T = SR.segment_table(pred, gt, C, connectivity, ignore)
        tp, fp, fn = BR.mask_counts_ref(pred, gt, C, ignore)
        s = T.sum(1)
        assert np.array_equal(s[0, 2], tp) and np.array_equal(s[0, 1], tp + fn)
        assert np.array_equal(s[1, 1], tp + fp) and np.array_equal(s[1, 2], tp)
        assert (T[:, :, 3] <= T[:, :, 0]).all() and (T[:, :, 2] <= T[:, :, 1]).all()
    assert np.array_equal(SR.segment_tables([], [pred, gt], gt, C, connectivity)[1, 0], SR.segment_tables([], [pred, gt], gt, C, connectivity)[1, 1])


def test_bin_of():
    assert [SR.bin_of(s) for s in (1, 2, 3, 4, 7, 8)] == [0, 1, 1, 2, 2, 3]
    for k in range(1, 31):
        assert SR.bin_of(2 ** k - 1) == min(k - 1, 23) and SR.bin_of(2 ** k) == min(k, 23)
        assert SR.bin_of(2 ** k) == min(int(math.floor(math.log2(2 ** k))), 23)
    assert SR.bin_of(2 ** 23) == 23 and SR.bin_of(2 ** 31 - 1) == 23 and SR.BINS == 24


def test_the_python_constants_restate_the_headers():
    from dasac_hip import ops
    index = open(os.path.join(ROOT, "da-sac_amd", "csrc", "segments_index.hpp")).read()
    tile = re.search(r"kTileH = (\d+), kTileW = (\d+);", index)
    assert ops.SEGMENT_TILE == (int(tile.group(1)), int(tile.group(2)))
    header = open(os.path.join(ROOT, "include", "dasac_hip.h")).read()
    bins = int(re.search(r"#define DASAC_SEGMENT_BINS (\d+)", header).group(1))
    assert ops.SEGMENT_BINS == bins == SR.BINS == int(re.search(r"kBins = (\d+);", index).group(1))
    assert ops.SEGMENT_ROWS == ("segments", "pixels", "matched_pixels", "matched_segments") == SR.ROWS


def test_summarise_and_format_segments_on_a_hand_written_table():
    import driver
    import reports
    assert driver.summarise_segments is reports.summarise_segments and driver.format_segments is reports.format_segments
    C = 3
    T = torch.zeros(2, 24, 4, C, dtype=torch.int64)
    # class 0: ten ground-truth segments of 4..7 pixels (bin 2), six found; two of 2048 pixels (bin 11), both found
    T[0, 2, :, 0] = torch.tensor([10, 50, 30, 6])
    T[0, 11, :, 0] = torch.tensor([2, 4096, 4000, 2])
    # predicted: forty specks of one pixel (bin 0), four of them real; three large segments, two real
    T[1, 0, :, 0] = torch.tensor([40, 40, 4, 4])
    T[1, 11, :, 0] = torch.tensor([3, 5000, 4026, 2])
    # class 1: one huge ground-truth segment in the last bin, found by one predicted segment; class 2: nothing at all
    T[0, 23, :, 1] = torch.tensor([1, 2 ** 24, 2 ** 24 - 5, 1])
    T[1, 23, :, 1] = torch.tensor([1, 2 ** 24, 2 ** 24 - 5, 1])
    S = driver.summarise_segments({"logits_up": T})
    assert list(S) == ["logits_up"] and list(S["logits_up"]) == ["< 64", "64-1023", "1024-16383", ">= 16384"]
    small, mid, large, huge = (S["logits_up"][k] for k in S["logits_up"])
    assert small["gt_segments"].tolist() == [10, 0, 0] and small["pred_segments"].tolist() == [40, 0, 0]
    assert small["object_recall"][0] == 0.6 and small["pixel_recall"][0] == 0.6 and small["segment_precision"][0] == 0.1
    assert small["unmatched_share"][0] == 0.9 and small["fragmentation"][0] == 4.0
    assert all(math.isnan(small[k][c]) for k in ("object_recall", "pixel_recall", "segment_precision", "unmatched_share", "fragmentation")
               for c in (1, 2))                                                # a class with no segment: NaN, not 0
    assert int(mid["gt_segments"].sum()) == 0 and math.isnan(mid["all_object_recall"])
    assert large["gt_segments"].tolist() == [2, 0, 0] and large["object_recall"][0] == 1.0 and large["fragmentation"][0] == 1.5
    assert abs(large["segment_precision"][0] - 2 / 3) < 1e-15
    assert huge["gt_segments"].tolist() == [0, 1, 0] and huge["object_recall"][1] == 1.0 and huge["all_gt_segments"] == 1
    assert small["all_gt_segments"] == 10 and small["all_pred_segments"] == 40 and small["all_object_recall"] == 0.6
    ignored = driver.summarise_segments({"logits_up": T}, ignore_classes=[0])["logits_up"]
    assert ignored["< 64"]["all_gt_segments"] == 0 and math.isnan(ignored["< 64"]["all_object_recall"])
    assert ignored["< 64"]["gt_segments"].tolist() == [10, 0, 0]                # the per-class rows keep every class
    two = driver.summarise_segments({"a": T, "b": T}, edges=(2, 4096))
    assert list(two["a"]) == ["< 2", "2-4095", ">= 4096"] and two["a"]["< 2"]["pred_segments"].tolist() == [40, 0, 0]
    assert two["b"]["2-4095"]["gt_segments"].tolist() == [12, 0, 0]
    for bad in ((64, 1000), (0, 64), (1024, 64), (3,)):
        with pytest.raises(ValueError):
            driver.summarise_segments({"logits_up": T}, edges=bad)
    with pytest.raises(ValueError):
        driver.summarise_segments({"logits_up": T[:, :23]})
    text = driver.format_segments(S, ["road", "pole", "sign"])
    assert len(text.splitlines()) == 1 + 4 + 1 + C and "nan" in text
    assert len(driver.format_segments(two, ["road", "pole", "sign"]).splitlines()) == 2 * (1 + 3 + 1 + C)


def test_the_new_arguments_default_to_off():
    import driver
    from dasac_hip import lib, ops
    params = inspect.signature(driver.validation).parameters
    assert params["segment_tables"].default is False and params["segment_connectivity"].default == 8
    assert inspect.signature(driver.despeckle).parameters["min_size"].default is inspect.Parameter.empty
    assert inspect.signature(ops.label_segments).parameters["connectivity"].default == 8
    assert inspect.signature(ops.segment_filter).parameters["fill"].default == 255
    for name in ("dasac_label_segments", "dasac_segment_counts", "dasac_segment_filter"):
        assert name in lib.PROTOTYPES and name + "_workspace" in lib.PROTOTYPES
    with pytest.raises(lib.DasacError, match="label_segments"):
        ops.label_segments(torch.zeros(1, 4, 4, dtype=torch.int64), 19)
    with pytest.raises(lib.DasacError, match="segment_filter"):
        ops.segment_filter(torch.zeros(1, 4, 4, dtype=torch.uint8), 4, 19)
    with pytest.raises(lib.DasacError, match="segment_counts"):
        ops.segment_counts([], [torch.zeros(1, 4, 4, dtype=torch.int64)], torch.zeros(1, 4, 4, dtype=torch.int64), num_classes=19)
