"""Importance-sampling weights and the target image selection (da-sac_amd/sampling.py) without a GPU, against golden g18
(tests/golden/make_goldens_sampling.py: the reference's compute_IS_weights.count, DataTarget.init_sampling and the selection
lines of DataTarget.__getitem__ on 12 synthetic label maps).  Everything is float64 / python floats in the reference's order
of operations: equality is exact."""
import bisect
import random
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import sampling

NUM_CLASSES = 19


def g18_maps(g):
    return [g["labels%d" % n] for n in range(len(g["names"]))]


def g18_counts(g):
    return np.stack([np.bincount(m.ravel(), minlength=256) for m in g18_maps(g)]).astype(np.int64)


def g18_weights(g, numpy_scalars=False):
    """The reference's weights dict rebuilt from the dense arrays, in the order of the file the tool wrote."""
    names = [str(n) for n in g["names"]]
    key, val = (np.uint8, np.float64) if numpy_scalars else (int, float)
    return {names[n]: {key(v): val(g["weights"][n, v]) for v in np.flatnonzero(g["present"][n])} for n in g["file_order"]}


def assert_weights_equal_golden(weights, g):
    names = [str(n) for n in g["names"]]
    assert list(weights) == names
    for n, name in enumerate(names):
        want = {int(v): float(g["weights"][n, v]) for v in np.flatnonzero(g["present"][n])}
        assert set(weights[name]) == set(want), name
        assert all(type(k) is int and type(v) is float for k, v in weights[name].items())
        for k in want:
            assert weights[name][k] == want[k], (name, k, weights[name][k], want[k])      # bit for bit
        assert 255 not in weights[name]


def test_fixture_meets_the_reference_preconditions(golden):
    g = golden("g18_is_sampling")
    counts = g18_counts(g)
    assert (counts[:, :NUM_CLASSES].sum(0) > 0).all(), "every class must occur (the reference asserts otherwise)"
    assert counts[:, NUM_CLASSES:255].sum() == 0
    assert len({m.shape for m in g18_maps(g)}) > 6, "different sizes"
    assert (counts[:, :255].sum(1) == 0).sum() == 1, "one image entirely 255"
    frac = counts[:, 255].sum() / counts.sum()
    assert 0.05 < frac < 0.3


def test_weights_from_counts_equal_the_reference_tool(golden):
    g = golden("g18_is_sampling")
    names = [str(n) for n in g["names"]]
    w = sampling.weights_from_counts(names, g18_counts(g))
    assert_weights_equal_golden(w, g)
    empty = [n for n in names if not w[n]]
    assert len(empty) == 1 and (g18_maps(g)[names.index(empty[0])] == 255).all()
    # order of the images does not matter (integer totals), tensors are taken too
    perm = np.random.RandomState(0).permutation(len(names))
    w2 = sampling.weights_from_counts([names[i] for i in perm], torch.from_numpy(g18_counts(g)[perm]))
    assert {k: w2[k] for k in names} == w
    with pytest.raises(ValueError):
        sampling.weights_from_counts(names[:-1], g18_counts(g))


@pytest.mark.parametrize("tag", ["none", "synthia"])
def test_init_sampling_equals_the_reference_tables(golden, tag):
    g = golden("g18_is_sampling")
    names = [str(n) for n in g["names"]]
    ignore = [] if tag == "none" else [int(c) for c in g["ignore_synthia"]]
    index = {n: i for i, n in enumerate(names)}
    for weights in (g18_weights(g), sampling.weights_from_counts(names, g18_counts(g))):
        tables = sampling.init_sampling(len(names), weights, index, NUM_CLASSES, ignore, float(g["prior_weight"]))
        assert len(tables) == NUM_CLASSES and all(len(t) == len(names) for t in tables)
        assert all(type(x) is float for t in tables for x in t)
        assert np.array_equal(np.array(tables, np.float64), g["tables_" + tag])          # bit for bit


def test_uniform_tables(golden):
    g = golden("g18_is_sampling")
    n = len(g["names"])
    tables = sampling.init_sampling(n, None, {}, NUM_CLASSES, [9], 0.25)
    assert np.array_equal(np.array(tables), g["tables_uniform"])
    want = [1. / n for _ in range(n)]
    for i in range(1, n):
        want[i] += want[i - 1]
    assert all(t == want for t in tables)


@pytest.mark.parametrize("tag", ["none", "synthia"])
def test_target_sampler_reproduces_every_recorded_selection(golden, tag):
    g = golden("g18_is_sampling")
    tables = [list(map(float, row)) for row in g["tables_" + tag]]
    for seed, want in zip(g["select_seeds"], g["select_" + tag]):
        s = sampling.TargetSampler(tables, random.Random(int(seed)))
        assert [s.select(i) for i in range(len(want))] == [int(x) for x in want]
    # the module-level `random` is the default stream, like the reference
    random.seed(int(g["select_seeds"][1]))
    s = sampling.TargetSampler(tables)
    assert [s.select(i) for i in range(64)] == [int(x) for x in g["select_" + tag][1]]


def test_select_clamps_a_draw_at_the_upper_end():
    class Top:
        def uniform(self, a, b):
            return b + 1e-9
    s = sampling.TargetSampler([[0.25, 0.5, 1.0]], Top())
    assert bisect.bisect_left(s.tables[0], 1.0 + 1e-9) == 3          # the reference would index past the end
    assert s.select(0) == 2


def test_save_and_load(golden, tmp_path):
    g = golden("g18_is_sampling")
    names = [str(n) for n in g["names"]]
    w = sampling.weights_from_counts(names, g18_counts(g))
    path = str(tmp_path / "weights.data")
    sampling.save_weights(path, w)
    assert torch.load(path) == w                                     # default arguments: weights_only=True
    assert sampling.load_weights(path) == w
    with pytest.raises(FileExistsError):
        sampling.save_weights(path, w)
    # a file as the reference tool writes it: numpy-scalar keys and values
    ref_path = str(tmp_path / "reference.data")
    torch.save(g18_weights(g, numpy_scalars=True), ref_path)
    loaded = sampling.load_weights(ref_path)
    assert all(type(k) is int and type(v) is float for stat in loaded.values() for k, v in stat.items())
    index = {n: i for i, n in enumerate(names)}
    tables = sampling.init_sampling(len(names), loaded, index, NUM_CLASSES, [], float(g["prior_weight"]))
    assert np.array_equal(np.array(tables), g["tables_none"])


def test_init_sampling_assertions(golden):
    g = golden("g18_is_sampling")
    names = [str(n) for n in g["names"]]
    w = g18_weights(g)
    index = {n: i for i, n in enumerate(names)}
    with pytest.raises(AssertionError, match="do not match"):
        sampling.init_sampling(len(names) + 1, w, index, NUM_CLASSES)
    # a class that occurs in no image: its cumulative table ends at prior_weight
    missing = {n: {k: v for k, v in stat.items() if k != 7} for n, stat in w.items()}
    with pytest.raises(AssertionError, match=r"\[7\].*class 7 .*VAL\.IGNORE_CLASS"):
        sampling.init_sampling(len(names), missing, index, NUM_CLASSES)
    tables = sampling.init_sampling(len(names), missing, index, NUM_CLASSES, ignore_classes=[7])
    assert tables[7] == sampling.init_sampling(len(names), None, index, NUM_CLASSES)[7]


def test_from_cfg(golden, tmp_path, capsys):
    g = golden("g18_is_sampling")
    names = [str(n) for n in g["names"]]
    path = str(tmp_path / "w.data")
    sampling.save_weights(path, g18_weights(g))
    cfg = lambda p, ign: NS(DATASET=NS(SAMPLE_WEIGHTS=p, SAMPLE_UNIFORM_PRIOR=float(g["prior_weight"])), VAL=NS(IGNORE_CLASS=ign))
    s = sampling.TargetSampler.from_cfg(cfg(path, [9, 14, 16]), names)
    assert "Loading sample weights" in capsys.readouterr().out
    assert np.array_equal(np.array(s.tables), g["tables_synthia"])
    s = sampling.TargetSampler.from_cfg(cfg("", []), names, g18_weights(g))
    assert np.array_equal(np.array(s.tables), g["tables_none"])
    s = sampling.TargetSampler.from_cfg(cfg(str(tmp_path / "nothing.data"), []), names)
    assert "Path to sample weights NOT found" in capsys.readouterr().out
    assert np.array_equal(np.array(s.tables), g["tables_uniform"])
    s = sampling.TargetSampler.from_cfg(cfg("", []), names)
    assert np.array_equal(np.array(s.tables), g["tables_uniform"])


def test_target_crops_select_draws_first(golden):
    import crops
    g = golden("g18_is_sampling")
    tables = [list(map(float, row)) for row in g["tables_none"]]
    sampler = sampling.TargetSampler(tables)
    kw = dict(group_size=2, seed=11, zoom_range=(0.5, 1.0))
    tc = crops.TargetCrops((64, 96), sampler=sampler, **kw)
    by_hand = crops.TargetCrops((64, 96), **kw)
    plain = random.Random(11)
    assert tc.rng.getstate() == plain.getstate()
    index = 5
    got = tc.select(index)
    r = plain.uniform(0, tables[index % NUM_CLASSES][-1])
    assert tc.rng.getstate() == plain.getstate()                     # exactly one uniform draw, from the TargetCrops' own rng
    assert got == bisect.bisect_left(tables[index % NUM_CLASSES], r)
    by_hand.rng.uniform(0, 1.0)
    assert tc.sample() == by_hand.sample()
    assert tc.views.sample() == by_hand.views.sample()
    # without a sampler nothing changes, and select says what is missing
    with pytest.raises(ValueError, match="sampler"):
        by_hand.select(0)
