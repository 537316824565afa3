"""The definitions behind `dasac_boundary_counts` without a GPU: the vectorised numpy model of tests/boundary_ref.py against a
per-pixel brute force, the window min / max equivalence the header states, the separable form the kernel computes (row table,
then column scan), the five slot-sum invariants against plain mask-count rules, and `driver.summarise_boundary` /
`driver.format_boundary` on hand-written tables."""
import numpy as np
import pytest
import torch

import boundary_ref as BR


def _maps(seed, B=2, C=5, H=13, W=17):
    rng = np.random.default_rng(seed)
    gt = BR.blocky((B, H, W), list(range(C)) + [255, -1], 4, rng)
    gt[1] = rng.integers(0, C, (H, W))                                  # a busy image beside a blocky one
    gt[0, 5:8, 2:9] = 255
    pred = BR.blocky((B, H, W), list(range(C)) + [255], 3, rng)
    pred[1, :, : W // 2] = gt[1, :, : W // 2]
    return gt, pred, C


@pytest.mark.parametrize("R", [1, 3, 16])
def test_model_distances_match_a_per_pixel_brute_force(R):
    for seed in (1, 2):
        gt, pred, C = _maps(seed)
        for m in (gt, pred):
            assert np.array_equal(BR.distances(m, C, R), BR.brute_force_distances(m, C, R))
    uniform = np.full((1, 6, 7), 3)
    assert (BR.distances(uniform, 5, R) == R + 1).all()                  # the image border is no contour
    assert (BR.distances(np.full((1, 6, 7), 255), 5, R) == R + 1).all()


@pytest.mark.parametrize("R", [1, 2, 5])
def test_distance_at_most_r_exactly_when_window_min_and_max_differ(R):
    gt, _, C = _maps(3)
    cls = BR.class_index(gt, C)
    d = BR.distances(gt, C, R)
    for r in range(1, R + 1):
        wmin, wmax = np.full(cls.shape, C), np.full(cls.shape, -1)     # over the class pixels of the window: no class is neither
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                s = BR._shifted(cls, dy, dx)
                wmin, wmax = np.minimum(wmin, np.where(s >= 0, s, C)), np.maximum(wmax, s)
        assert np.array_equal((d <= r), (cls >= 0) & (wmin != wmax)), r


def _separable_distances(labels, C, R):
    """The kernel's two passes, restated: per pixel of a row the class k1 of the nearest class pixel of the row, its distance d1 and
    the distance d2 of the nearest pixel of the row with a class other than k1; then d = min over |dy| <= R of
    max(|dy|, c != k1 ? d1 : d2)."""
    cls = BR.class_index(labels, C)
    B, H, W = cls.shape
    k1, d1, d2 = np.full(cls.shape, -1), np.full(cls.shape, R + 1), np.full(cls.shape, R + 1)
    for b in range(B):
        for y in range(H):
            for x in range(W):
                for dx in range(R + 1):
                    for xx in (x - dx, x + dx):
                        v = cls[b, y, xx] if 0 <= xx < W else -1
                        if v < 0:
                            continue
                        if k1[b, y, x] < 0:
                            k1[b, y, x], d1[b, y, x] = v, dx
                        elif v != k1[b, y, x] and d2[b, y, x] > R:
                            d2[b, y, x] = dx
    d = np.full(cls.shape, R + 1)
    for b in range(B):
        for y in range(H):
            for x in range(W):
                if cls[b, y, x] < 0:
                    continue
                for yy in range(max(0, y - R), min(H, y + R + 1)):
                    rd = d1[b, yy, x] if k1[b, yy, x] != cls[b, y, x] else d2[b, yy, x]
                    d[b, y, x] = min(d[b, y, x], max(abs(yy - y), rd))
    return d


@pytest.mark.parametrize("R", [1, 4, 16])
def test_separable_row_then_column_form_is_the_definition(R):
    for seed in (4, 5):
        gt, pred, C = _maps(seed)
        for m in (gt, pred):
            assert np.array_equal(_separable_distances(m, C, R), BR.distances(m, C, R))


@pytest.mark.parametrize("R,ignore", [(1, 255), (4, 255), (16, 255), (4, 2)])
def test_slot_sums_are_the_plain_counts(R, ignore):
    gt, pred, C = _maps(6)
    T = BR.boundary_table(pred, gt, C, R, ignore)
    plain = BR.mask_counts_ref(pred, gt, C, ignore)
    s = T.sum(0)
    assert np.array_equal(s[0], plain[0]) and np.array_equal(s[1], plain[1]) and np.array_equal(s[2], plain[2])
    assert np.array_equal(s[3], plain[0] + plain[1]) and np.array_equal(s[4], plain[0])
    assert T[:R].sum() > 0
    if R == 1:
        assert T[R].sum() > 0                                           # blocks of 3 and 4: their centres are further than 1 from a contour
    # a perfect prediction: pred and both are tp, slot by slot
    P = BR.boundary_table(gt, gt, C, R, ignore)
    assert np.array_equal(P[:, 3], P[:, 0]) and np.array_equal(P[:, 4], P[:, 0]) and P[:, 1:3].sum() == 0


def _stripes(shift=0, B=1, C=3, H=12, W=30):
    """Vertical stripes 10 wide, classes 0 1 2; `shift` moves the contours right."""
    x = np.clip((np.arange(W) - shift) // 10, 0, C - 1)
    return np.broadcast_to(x, (B, H, W)).copy()


def test_summarise_boundary_perfect_prediction_scores_one_everywhere():
    import driver
    C, R = 3, 4
    T = torch.zeros(R + 1, 5, C, dtype=torch.int64)
    for s in range(R + 1):                                             # hand-written: tp == pred == both in every slot
        T[s, 0] = T[s, 3] = T[s, 4] = torch.tensor([10 + s, 20, 5])
    out = driver.summarise_boundary({"layer": T}, radii=(1, 2, 4))
    assert sorted(out["layer"]) == [1, 2, 4]
    for r, e in out["layer"].items():
        for key in ("band_iou", "interior_iou", "boundary_iou"):
            assert e[key].dtype == torch.float32 and torch.equal(e[key], torch.ones(C)), (r, key)
        assert e["band_miou"] == e["interior_miou"] == e["boundary_miou"] == 1.0
        assert e["error_share"] == 0.0
    assert out["layer"][1]["pixel_share"] == pytest.approx(35 / (35 * 5 + 10))
    text = driver.format_boundary(out, ["a", "b", "c"])
    assert "layer" in text and "r=4" in text and len(text.splitlines()) == 1 + 3 + 1 + C


def test_summarise_boundary_shifted_prediction_loses_only_in_slot_zero():
    import driver
    C, R = 3, 4
    gt, pred = _stripes(0), _stripes(1)
    T = BR.boundary_table(pred, gt, C, R)
    assert T[1:, 1:3].sum() == 0 and T[0, 1:3].sum() == 2 * 2 * 12      # every error touches a ground-truth contour
    out = driver.summarise_boundary({"shifted": torch.from_numpy(T)}, radii=(1, 2, 4))["shifted"]
    for r in (1, 2, 4):
        assert torch.equal(out[r]["interior_iou"], torch.ones(C)) and out[r]["error_share"] == 1.0
        assert float(out[r]["band_iou"].max()) < 1.0 and float(out[r]["boundary_iou"].max()) < 1.0
    assert out[1]["band_miou"] < out[2]["band_miou"] < out[4]["band_miou"] < 1.0
    # the band of width 1 by hand: class 0 keeps its 12 contour pixels and gains 12 false positives next door; class 1 has 24 pixels
    # in the band, loses 12 and gains 12; class 2 has 12 and loses them all
    want = torch.tensor([12 / 24, 12 / 36, 0 / 12], dtype=torch.float32)
    assert torch.allclose(out[1]["band_iou"], want, rtol=0, atol=1e-7)


def test_summarise_boundary_absent_class_scores_zero_and_ignored_classes_leave_the_means():
    import driver
    C, R = 4, 2
    T = torch.zeros(R + 1, 5, C, dtype=torch.int64)
    T[:, 0, :2] = T[:, 3, :2] = T[:, 4, :2] = 7                         # classes 2 and 3 never occur
    T[0, 1, 1] = 7                                                      # class 1: as many false positives as hits in slot 0
    T[0, 3, 1] += 7
    e = driver.summarise_boundary({"l": T}, radii=(1,))["l"][1]
    assert e["band_iou"].tolist() == [1.0, 0.5, 0.0, 0.0] and e["interior_iou"].tolist() == [1.0, 1.0, 0.0, 0.0]
    assert e["boundary_iou"].tolist() == [1.0, 0.5, 0.0, 0.0]
    assert e["band_miou"] == pytest.approx(0.375)
    kept = driver.summarise_boundary({"l": T}, ignore_classes=[2, 3], radii=(1,))["l"][1]
    assert kept["band_miou"] == pytest.approx(0.75) and torch.equal(kept["band_iou"], e["band_iou"])
    assert driver.summarise_iou(T.sum(0)[:3])[0].tolist() == [1.0, 0.75, 0.0, 0.0]          # the rule it follows


def test_summarise_boundary_refuses_radii_above_the_table():
    import driver
    T = torch.zeros(5, 5, 3, dtype=torch.int64)                          # R = 4
    driver.summarise_boundary({"l": T}, radii=(1, 4))
    with pytest.raises(ValueError):
        driver.summarise_boundary({"l": T})                              # the default radii reach 8
    with pytest.raises(ValueError):
        driver.summarise_boundary({"l": T}, radii=(5,))
    with pytest.raises(ValueError):
        driver.summarise_boundary({"l": T}, radii=(0,))


def test_the_new_keywords_exist():
    import inspect
    import driver
    from dasac_hip import lib, ops
    assert inspect.signature(driver.validation).parameters["boundary_radius"].default == 0
    assert inspect.signature(driver.validation_iou).parameters["boundary_radius"].default == 0
    assert inspect.signature(ops.boundary_counts).parameters["radius"].default == 8
    assert "dasac_boundary_counts" in lib.PROTOTYPES and "dasac_boundary_counts_workspace" in lib.PROTOTYPES
