"""Reference-form validation (driver.validation, train.py:339-469) -- the parts that need no GPU: the g19 fixture is consistent
with itself (counts recomputed in numpy from its stored layer maps give its stored counts, summaries and scores), and the
pure-host parts of the driver reproduce the reference's figures from the reference's counts."""
import numpy as np
import pytest
import torch

LAYERS = {"src": ["logits_up"], "tgt": ["logits_up", "teacher_init", "teacher_refined", "teacher_labels"]}
IGNORE = {"none": [], "synthia": [9, 14, 16]}


def recount(pred, gt, C=19, ignore_index=255):
    """utils/metrics.py:18-39 restated on integer maps: int64 [3,C] = (tp, fp, fn)."""
    pred, gt = np.asarray(pred).astype(np.int64).ravel(), np.asarray(gt).astype(np.int64).ravel()
    keep = gt != ignore_index
    pred, gt = pred[keep], gt[keep]
    hit = pred == gt
    out = np.zeros((3, C), np.int64)
    for c in range(C):
        out[0, c] = np.sum(hit & (gt == c))
        out[1, c] = np.sum(~hit & (pred == c))
        out[2, c] = np.sum(~hit & (gt == c))
    return out


@pytest.fixture(scope="module")
def g19(golden):
    return golden("g19_validation")


@pytest.mark.parametrize("name", ["src", "tgt"])
def test_fixture_counts_follow_from_its_own_layer_maps(g19, name):
    assert list(g19[name + "_layers"]) == LAYERS[name]
    counted = int(g19["counted"])
    assert counted == int(g19["max_iter"]) + 2 and int(g19["num_batches"]) > counted
    for layer in LAYERS[name]:
        total = sum(recount(g19["%s%d_%s_map" % (name, b, layer)], g19["%s%d_gt_seen" % (name, b)]) for b in range(counted))
        assert np.array_equal(total, g19["%s_%s_counts" % (name, layer)]), layer


def test_fixture_windows_follow_from_their_own_tensors(g19):
    total = {layer: np.zeros((3, 19), np.int64) for layer in LAYERS["tgt"]}
    for b in range(int(g19["win"][3])):
        for layer in LAYERS["tgt"]:
            t = g19["win%d_%s" % (b, layer)]
            total[layer] += recount(t if layer == "teacher_labels" else t.argmax(1), g19["win%d_gt" % b])
            assert np.array_equal(total[layer], g19["win%d_%s_counts" % (b, layer)]), (b, layer)


def test_fixture_is_not_vacuous(g19):
    labels = np.concatenate([g19["tgt%d_teacher_labels_map" % b].ravel() for b in range(3)])
    assert 0.2 <= np.mean(labels != 255) <= 0.8
    for name in LAYERS:
        for layer in LAYERS[name]:
            c = g19["%s_%s_counts" % (name, layer)]
            assert (c[1] > 0).any() and (c[2] > 0).any()
            low = np.concatenate([g19["%s%d_%s_margin" % (name, b, layer)].astype(np.float32).ravel() for b in range(3)]) < float(g19["contract"])
            assert low.mean() <= 0.01
    mious = [g19["tgt_%s_mean_none" % layer][0] for layer in LAYERS["tgt"]]
    assert min(abs(mious[0] - m) for m in mious[1:]) > 1e-3 and int(np.argmax(mious)) != 0      # the teacher holds the score
    assert any((g19["tgt%d_gt" % b] == -1).any() for b in range(3))                            # augmentation padding is present


@pytest.mark.parametrize("name", ["src", "tgt"])
@pytest.mark.parametrize("tag", ["none", "synthia"])
def test_summaries_class_subset_means_and_score_match_the_reference(g19, name, tag):
    import driver
    counts = {layer: torch.from_numpy(g19["%s_%s_counts" % (name, layer)]) for layer in LAYERS[name]}
    per_class, mean, score = driver.summarise_validation(counts, IGNORE[tag])
    for layer in LAYERS[name]:
        np.testing.assert_allclose(torch.stack(per_class[layer]).numpy(), g19["%s_%s_summary" % (name, layer)], rtol=1e-6, atol=0)
        np.testing.assert_allclose(mean[layer], g19["%s_%s_mean_%s" % (name, layer, tag)], rtol=1e-6, atol=0)
    assert score == pytest.approx(float(g19["%s_score_%s" % (name, tag)]), rel=1e-6)
    assert score == max(m[0] for m in mean.values())
    if name == "tgt":
        assert score != mean["logits_up"][0]              # a score that looked at the student alone would be caught


def test_class_subset_mean_drops_exactly_the_listed_classes():
    import driver
    v = torch.arange(19, dtype=torch.float32)
    assert driver.class_subset_mean(v) == pytest.approx(9.0)
    assert driver.class_subset_mean(v, [9, 14, 16]) == pytest.approx((171 - 39) / 16.0)
    assert driver.summarise_validation({}, [1]) == ({}, {}, 0.0)               # the score starts from 0.0 (train.py:408)


def test_stat_manager_mean():
    import driver
    assert driver.stat_mean([1.0, 2.0, 6.0]) == 3.0
    assert driver.stat_mean([]) == 0
    assert driver.stat_mean([2.5, -2.5]) == 0                                   # a sum of exactly 0 reads as 0 (stat_manager.py:57-61)
    assert driver.stat_mean([0.1] * 3) == (0.1 + 0.1 + 0.1) / 3                 # python-float accumulation, in order


def test_batch_count_rule(g19):
    """train.py:405-406 breaks on n > max_iter AFTER batch n: max_iter + 2 batches of a longer loader."""
    import driver
    loader = list(range(int(g19["num_batches"])))
    assert list(driver.validation_batches(loader, int(g19["max_iter"]))) == loader[:int(g19["counted"])]
    assert list(driver.validation_batches(loader, 0)) == loader[:2]
    assert list(driver.validation_batches(loader, None)) == loader              # defaults to len(loader): never reached
    assert list(driver.validation_batches(loader, 2)) == loader
    assert list(driver.validation_batches(iter(loader), None)) == loader        # no len(): no limit
    assert list(driver.validation_batches([], 1)) == []
