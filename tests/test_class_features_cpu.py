"""Host side of the class feature tables: the numpy reference of tests/class_features_ref.py against a brute-force loop, the
node rounding rule, and driver.class_gap_report / format_class_gap_report on tables the reference builds from planted data.
No GPU."""
from types import SimpleNamespace as NS

import numpy as np
import pytest

import class_features_ref as ref

SHARE_SHAPES = [((33, 49), (5, 7)), ((30, 52), (5, 8)), ((65, 65), (9, 9))]


def test_node_rounding_rule():
    assert [ref.node_pixel(i, 5, 33) for i in range(5)] == [0, 8, 16, 24, 32]
    assert [ref.node_pixel(i, 5, 30) for i in range(5)] == [0, 7, 15, 22, 29]          # 7.25, 14.5 (a half: up), 21.75
    assert [ref.node_pixel(i, 1, 17) for i in range(1)] == [0]
    assert [ref.node_pixel(i, 9, 9) for i in range(9)] == list(range(9))


def brute_nodes(lab, h, w, C, r):
    N, H, W = lab.shape
    out = np.zeros((N, h, w), dtype=np.uint8)
    for n in range(N):
        for i in range(h):
            for j in range(w):
                Y = 0 if h == 1 else int(np.floor(i * (H - 1) / (h - 1) + 0.5))
                X = 0 if w == 1 else int(np.floor(j * (W - 1) / (w - 1) + 0.5))
                v = int(lab[n, Y, X])
                ok = 0 <= v < C
                for y in range(Y - r, Y + r + 1):
                    for x in range(X - r, X + r + 1):
                        if 0 <= y < H and 0 <= x < W and int(lab[n, y, x]) != v:
                            ok = False
                out[n, i, j] = v if ok else 255
    return out


def test_reference_against_a_brute_force_loop():
    lab = ref.blocks(2, 30, 52, 19, seed=4)
    lab[1, 3, 3] = 200                                           # neither a class nor 255
    assert (lab == 255).sum() >= 54 and (lab == -1).sum() >= 4
    for r in (0, 1, 2, 4):
        for C in (19, 2):
            assert np.array_equal(ref.label_nodes(lab, 5, 8, C, r), brute_nodes(lab, 5, 8, C, r)), (r, C)
    assert np.array_equal(ref.label_nodes(lab.astype(np.uint8), 5, 8, 19, 2), ref.label_nodes(lab, 5, 8, 19, 2))      # -1 and 255: no class alike
    rng = np.random.RandomState(1)
    x = rng.randn(2, 3, 40).astype(np.float32)
    nodes = ref.label_nodes(lab, 5, 8, 19, 1)
    sums, counts, abs_sum, entries = ref.table(x, nodes, 19)
    want_s, want_c, want_a = np.zeros((19, 3, 2)), np.zeros(19, dtype=np.int64), np.zeros((19, 3))
    flat = nodes.reshape(2, 40)
    for n in range(2):
        for p in range(40):
            c = int(flat[n, p])
            if c < 19:
                want_c[c] += 1
                for f in range(3):
                    d = float(x[n, f, p])
                    want_s[c, f, 0] += d
                    want_s[c, f, 1] += d * d
                    want_a[c, f] += abs(d)
    assert np.array_equal(counts, want_c) and np.array_equal(entries, want_c)
    assert np.allclose(sums, want_s, rtol=1e-13, atol=0) and np.allclose(abs_sum, want_a, rtol=1e-13, atol=0)


@pytest.mark.parametrize("size,nodes_hw", SHARE_SHAPES)
def test_the_purity_window_bites_but_not_everywhere(size, nodes_hw):
    lab = ref.blocks(3, size[0], size[1], 19, seed=0)
    for r in (1, 2):
        share = ref.kept_share(ref.label_nodes(lab, nodes_hw[0], nodes_hw[1], 19, r))
        print("{} -> {}, r = {}: {:.2f} of the nodes keep a class".format(size, nodes_hw, r, share))
        assert 0.05 <= share <= 0.95, (size, r, share)


# ---------------------------------------------------------------------------------------------- the report
C, CF, POS = 6, 12, 400
MU = np.array([[3.0 * c + 0.5 * f for f in range(CF)] for c in range(C)])            # class prototypes, well apart
SIGMA = np.array([[0.5 + 0.1 * ((c + f) % 4) for f in range(CF)] for c in range(C)])


def planted(seed, drawn_from=None, sizes=None):
    """A table over one sample of C * POS positions: class c at positions c * POS .. c * POS + sizes[c] - 1, its features drawn
    from class drawn_from[c]'s distribution; channel 0 is dead (all zero) everywhere."""
    rng = np.random.RandomState(seed)
    drawn_from = list(range(C)) if drawn_from is None else drawn_from
    sizes = [POS] * C if sizes is None else sizes
    nodes = np.full((1, C * POS), 255, dtype=np.uint8)
    x = np.zeros((1, CF, C * POS), dtype=np.float32)
    for c in range(C):
        k = drawn_from[c]
        nodes[0, c * POS:c * POS + sizes[c]] = c
        x[0, :, c * POS:(c + 1) * POS] = (MU[k][:, None] + SIGMA[k][:, None] * rng.randn(CF, POS)).astype(np.float32)
    x[0, 0] = 0.0
    sums, counts, _, _ = ref.table(x, nodes, C)
    return NS(sums=sums, counts=counts), x, nodes


def test_a_table_against_itself_has_no_gap():
    import driver
    a, _, _ = planted(1)
    rep = driver.class_gap_report(a, a, min_nodes=16)
    assert rep["skipped"] == {} and (rep["gap"] == 0).all() and np.isinf(rep["margin"]).all()
    assert (np.diag(rep["matrix"]) == 0).all() and (rep["matrix"][~np.eye(C, dtype=bool)] > 0).all()
    alone = driver.class_gap_report(a)
    assert alone["within"] and (np.diag(alone["matrix"]) == 0).all() and np.array_equal(alone["matrix"], rep["matrix"])
    assert np.array_equal(alone["nearest"], rep["nearest"]) and len(alone["top"]) == 5


def test_a_class_drawn_from_another_is_nearest_to_that_one():
    import driver
    a, _, _ = planted(1)
    b, _, _ = planted(2, drawn_from=[0, 1, 4, 3, 4, 5])          # b's class 2 looks like a's class 4
    rep = driver.class_gap_report(a, b, top=3)
    assert rep["nearest"][2] == 4 and rep["margin"][2] < 1 and rep["top"][0] == 2 and len(rep["top"]) == 3
    others = [c for c in range(C) if c != 2]
    assert (rep["margin"][others] > 1).all() and (rep["gap"][others] < rep["gap"][2]).all()
    assert np.array_equal(rep["counts_a"], [POS] * C) and np.array_equal(rep["counts_b"], [POS] * C)
    text = driver.format_class_gap_report(rep, ["c{}".format(c) for c in range(C)])
    assert text.count("\n") == C + 1 and text.split("\n")[1].startswith("c2") and text.endswith("margin below 1: c2")


def test_small_and_ignored_classes_are_skipped_with_nan():
    import driver
    a, _, _ = planted(1)
    b, _, _ = planted(3, sizes=[POS, 15, POS, 0, POS, POS])
    rep = driver.class_gap_report(a, b, ignore_classes=(5,), min_nodes=16)
    assert rep["skipped"] == {1: "under min_nodes", 3: "absent", 5: "ignored"}
    for c in (1, 3, 5):
        assert np.isnan(rep["gap"][c]) and np.isnan(rep["margin"][c]) and np.isnan(rep["nearest_distance"][c]) and rep["nearest"][c] == -1
        assert np.isnan(rep["matrix"][c]).all()
    assert np.isnan(rep["matrix"][:, 5]).all() and not np.isnan(rep["matrix"][0, 1])      # a's class 1 counts as a neighbour, a's 5 does not
    for c in (0, 2, 4):
        assert np.isfinite(rep["gap"][c]) and rep["nearest"][c] not in (c, 5)
    assert driver.format_class_gap_report(rep).count("\n") == 3 + 1
    assert driver.class_gap_report(a, b, min_nodes=15)["skipped"] == {3: "absent"}
    with pytest.raises(ValueError):
        driver.class_gap_report(a, NS(sums=a.sums[:, :5], counts=a.counts))


def test_distance_is_the_domain_gap_formula():
    """D of two class rows against driver.domain_gap_report on two activation tables holding the same two rows (equal node counts,
    as that report takes one element count per layer): its per-layer `gap` is the mean over the channels not dead in both, its
    gap_max the largest per-channel term."""
    import driver
    a, xa, na = planted(1)
    b, xb, nb = planted(2)
    rep = driver.class_gap_report(a, b)
    layout = [dict(op=-1, slot=0, name="input", kind="input", C=CF, H=POS, W=1, relu=False, row0=0)]

    def activation_record(sums, x):
        t = np.zeros((1, CF, 6))
        t[0, :, 0], t[0, :, 1] = sums[:, 0], sums[:, 1]
        t[0, :, 5] = (x == 0).sum(axis=1)
        return driver.ActivationRecord("backbone", 1, (0, 1), t, layout)
    for c, k in [(0, 0), (2, 2), (1, 4), (5, 3)]:
        ra = activation_record(a.sums[k], xa[0][:, na[0] == k])
        rb = activation_record(b.sums[c], xb[0][:, nb[0] == c])
        layer = driver.domain_gap_report(rb, ra)["layers"][0]
        assert layer["dead_both"] == 1
        assert abs(rep["matrix"][c, k] - layer["gap"]) <= 1e-12 * layer["gap"], (c, k)
        mu_a, mu_b = a.sums[k][:, 0] / POS, b.sums[c][:, 0] / POS
        var_a, var_b = np.maximum(a.sums[k][:, 1] / POS - mu_a ** 2, 0), np.maximum(b.sums[c][:, 1] / POS - mu_b ** 2, 0)
        per_channel = driver.moment_gap(mu_b, var_b, mu_a, var_a)
        assert abs(per_channel.max() - layer["gap_max"]) <= 1e-12 * layer["gap_max"] and int(np.argmax(per_channel)) == layer["gap_max_channel"]


def test_new_entry_points_are_declared_and_bound():
    import ctypes
    from dasac_hip import lib as L
    from dasac_hip import ops
    assert L.PROTOTYPES["dasac_class_feature_stats_workspace"] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    assert len(L.PROTOTYPES["dasac_class_feature_stats"][1]) == 11 and len(L.PROTOTYPES["dasac_label_nodes"][1]) == 11
    assert ops.CLASS_FEATURE_COLUMNS == ref.COLUMNS == ("sum", "sumsq")
    lib = L.load()
    assert lib.dasac_class_feature_stats_workspace(16, 2048, 19) == 16 * 2048 * 19 * 16
    assert lib.dasac_class_feature_stats_workspace(0, 4, 19) == 0


def test_ops_refuse_cpu_tensors_and_the_engine_lists_its_names():
    import torch
    from dasac_hip import DasacError, ops
    with pytest.raises(DasacError):
        ops.label_nodes(torch.zeros(1, 8, 8, dtype=torch.int64), (2, 2), 19)
    with pytest.raises(DasacError):
        ops.class_feature_stats(torch.zeros(1, 2, 4), torch.zeros(1, 4, dtype=torch.uint8), 19)
    import models
    import torch.nn as nn
    net = models.DeepLabV2_ResNet101(num_classes=19, criterion=nn.CrossEntropyLoss(ignore_index=255, reduction="none"), freeze_bn=True)
    from dasac_hip import engine as E
    eng = E.Engine(net._plan())
    assert eng.tap is None
    names = {m: n for n, m in net.named_modules()}
    index, name = eng.tap_index(None, names)
    assert name == "model.layer4.2" or name.startswith("model.layer4.2."), name
    assert eng.plan.ops[index].dst == eng.plan.ops[-1].src and index == len(eng.plan.ops) - 2
    assert eng.tap_index("input", names) == (-1, "input")
    assert eng.tap_index("model.conv1", names) == (0, "model.conv1")
    with pytest.raises(ValueError) as err:
        eng.tap_index("no.such.layer", names)
    assert "model.conv1" in str(err.value) and "input" in str(err.value)
