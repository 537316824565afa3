"""Host side of the per-layer activation tables (no GPU): `driver.activation_report` / `domain_gap_report` and their formatters
over hand-built tables, the descriptor layout of `ops.ActivationStatsPlan`, the segment bounds the Python layer refuses, the
layout names of an engine, and the host-side refusals of dasac_activation_stats."""
import ctypes
import math

import numpy as np
import pytest
import torch

import activation_stats_ref as ref


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as ge
    ge.build()


def entry(op, slot, name, kind, C, H, W, relu, row0):
    return dict(op=op, slot=slot, name=name, kind=kind, C=C, H=H, W=W, relu=relu, row0=row0)


# two tensors: "input" [N=3, C=2, 2x2] and "conv" [3, 3, 1x2]; two segments (samples 0 and 1..2)
LAYOUT = [entry(-1, 0, "input", "input", 2, 2, 2, False, 0), entry(0, 1, "conv", "conv", 3, 1, 2, True, 2)]
N, BOUNDS = 3, (0, 1, 3)


def rows_of(values):
    """[sum, sumsq, maxabs, nonfinite, first, zeros] of a list of finite values."""
    v = np.asarray(values, dtype=np.float64)
    return [v.sum(), (v * v).sum(), np.abs(v).max() if len(v) else 0.0, 0.0, 0.0, float((v == 0).sum())]


def hand_table():
    """Segment 0 holds 4 (input) / 2 (conv) elements per channel, segment 1 twice as many."""
    T = np.zeros((2, 5, 6))
    # input channel 0: mean 2.5, var 1.25 in segment 0; mean 5, var 4 in segment 1
    T[0, 0] = rows_of([1, 2, 3, 4])
    T[1, 0] = rows_of([3, 3, 3, 3, 7, 7, 7, 7])
    # input channel 1: a constant channel in both segments (den == 0, num > 0)
    T[0, 1] = rows_of([2, 2, 2, 2])
    T[1, 1] = rows_of([3] * 8)
    # conv channel 0: dead in segment 0 only; channel 1: dead in both; channel 2: alive, identical statistics
    T[0, 2] = rows_of([0, 0])
    T[1, 2] = rows_of([1, 0, 2, 0])
    T[0, 3] = rows_of([0, 0])
    T[1, 3] = rows_of([0, 0, 0, 0])
    T[0, 4] = rows_of([1, 3])
    T[1, 4] = rows_of([1, 3, 1, 3])
    return T


def record(T, layout=LAYOUT, bounds=BOUNDS, n=N, net="backbone"):
    import driver
    return driver.ActivationRecord(net, n, bounds, torch.from_numpy(np.ascontiguousarray(T)), layout)


def test_activation_report_reads_means_variances_zero_shares_and_dead_channels():
    import driver
    rep = driver.activation_report(record(hand_table()), segment=0)
    assert [l["name"] for l in rep["layers"]] == ["input", "conv"] and rep["net"] == "backbone" and rep["samples"] == (0, 1)
    inp, conv = rep["layers"]
    assert inp["shape"] == (1, 2, 2, 2) and conv["shape"] == (1, 3, 1, 2) and (inp["kind"], conv["kind"]) == ("input", "conv")
    vals = np.asarray([1, 2, 3, 4, 2, 2, 2, 2], dtype=np.float64)
    assert inp["mean"] == vals.mean() and math.isclose(inp["std"], vals.std(), rel_tol=1e-15) and inp["maxabs"] == 4.0
    assert inp["zero_share"] == 0.0 and inp["dead_channels"] == 0 and inp["nonfinite"] == 0 and inp["first_nonfinite"] is None
    assert conv["zero_share"] == 4.0 / 6.0 and conv["dead_channels"] == 2 and conv["maxabs"] == 3.0
    assert rep["first_nonfinite_layer"] is None and rep["top"] == ["input", "conv"]
    seg1 = driver.activation_report(record(hand_table()), segment=1, top=1)
    assert seg1["samples"] == (1, 3) and seg1["layers"][1]["dead_channels"] == 1 and seg1["layers"][1]["shape"] == (2, 3, 1, 2)
    assert seg1["layers"][0]["maxabs"] == 7.0 and seg1["top"] == ["input"]


def test_activation_report_unravels_planted_first_nonfinite_indices():
    import driver
    T = hand_table()
    # conv [3, 3, 1, 2]: flat index of (n=2, c=1, y=0, x=1) is (2*3 + 1)*2 + 1 = 15, of (1, 2, 0, 0) it is 10
    T[1, 3, 3:5] = (1, 16)
    T[1, 4, 3:5] = (2, 11)
    rep = driver.activation_report(record(T), segment=1)
    assert rep["first_nonfinite_layer"] == "conv" and rep["layers"][0]["first_nonfinite"] is None
    assert rep["layers"][1]["nonfinite"] == 3 and rep["layers"][1]["first_nonfinite"] == (1, 2, 0, 0)
    # the mean runs over the finite entries: 12 elements, 3 of them non-finite
    assert rep["layers"][1]["mean"] == (3.0 + 0.0 + 8.0) / 9.0
    # both layers bad: the first in plan order is named; input [3, 2, 2, 2]: (0, 1, 1, 0) is flat 6
    T[0, 1, 3:5] = (1, 7)
    rep0 = driver.activation_report(record(T), segment=0)
    assert rep0["first_nonfinite_layer"] == "input" and rep0["layers"][0]["first_nonfinite"] == (0, 1, 1, 0)
    assert driver.activation_report(record(T), segment=1)["first_nonfinite_layer"] == "conv"


def test_domain_gap_report_known_values_dead_and_constant_channels():
    import driver
    rep = driver.domain_gap_report(record(hand_table()))
    inp, conv = rep["layers"]
    g0 = ref.gap(2.5, 1.25, 5.0, 4.0)
    assert g0 == (2.5 ** 2 + (math.sqrt(1.25) - 2.0) ** 2) / (0.5 * 5.25)
    g1 = 1.0 / 1e-30                                         # constant channel: num = 1, den = 0
    assert inp["gap_max"] == g1 and inp["gap_max_channel"] == 1 and inp["gap"] == (g0 + g1) / 2
    assert inp["mean_shift"] == math.sqrt((2.5 ** 2 + 1.0) / 2)
    assert (inp["dead_only_a"], inp["dead_only_b"], inp["dead_both"]) == (0, 0, 0)
    # conv: channel 0 dead in a only (mu_b = 0.75, var_b = 1.25 - 0.5625), channel 1 dead in both (left out), channel 2 identical
    gc0 = ref.gap(0.0, 0.0, 0.75, 1.25 - 0.5625)
    assert (conv["dead_only_a"], conv["dead_only_b"], conv["dead_both"]) == (1, 0, 1)
    assert conv["gap"] == (gc0 + 0.0) / 2 and conv["gap_max"] == gc0 and conv["gap_max_channel"] == 0
    assert conv["mean_shift"] == math.sqrt(0.75 ** 2 / 3)
    assert rep["top"] == ["input", "conv"]
    # two records, segment 0 of each: identical tables give exactly 0 everywhere
    T = hand_table()
    same = driver.domain_gap_report(record(T[:1], bounds=(0, 1), n=1), record(T[:1].copy(), bounds=(0, 1), n=1))
    assert all(l["gap"] == 0.0 and l["gap_max"] == 0.0 and l["mean_shift"] == 0.0 for l in same["layers"])
    assert same["layers"][1]["dead_both"] == 2
    # and two records of different batch sizes compare per element
    two = driver.domain_gap_report(record(T[:1], bounds=(0, 1), n=1), record(T[1:], bounds=(0, 2), n=2))
    assert two["layers"][0]["gap"] == inp["gap"] and two["layers"][1]["gap"] == conv["gap"]


def test_domain_gap_report_refuses_mismatched_layouts_and_single_segments():
    import driver
    T = hand_table()
    other = [dict(LAYOUT[0]), dict(LAYOUT[1], name="conv2")]
    with pytest.raises(ValueError):
        driver.domain_gap_report(record(T), record(T, layout=other))
    with pytest.raises(ValueError):
        driver.domain_gap_report(record(T), record(T[:, :4], layout=[LAYOUT[0], dict(LAYOUT[1], C=2)]))
    with pytest.raises(ValueError):
        driver.domain_gap_report(record(T[:1], bounds=(0, 3)))          # one record, one segment


def test_formatters_give_one_line_per_row_with_stable_columns():
    import driver
    T = hand_table()
    T[1, 4, 3:5] = (2, 11)
    rep = driver.activation_report(record(T), segment=1, top=1)
    text = driver.format_activation_report(rep, top=1).split("\n")
    assert len(text) == 4                                    # header, the top layer, the layer with non-finite entries, the summary
    assert text[0].split() == ["layer", "kind", "shape", "mean", "std", "max|x|", "zeros", "dead", "nonfinite", "first"]
    assert text[1].split()[:3] == ["input", "input", "2x2x2x2"] and text[1].split()[-2:] == ["0", "-"]
    assert text[2].split()[:3] == ["conv", "conv", "2x3x1x2"] and text[2].endswith("2 (1, 2, 0, 0)")
    assert text[3] == "backbone segment 1 (samples 1..2): 2 layers; first layer with non-finite entries: conv"
    ends = [len(line) for line in text[:2]]
    assert ends[0] == ends[1]                                # right-aligned columns: the rows end where the header ends
    assert text == driver.format_activation_report(rep, top=1).split("\n")
    gap = driver.domain_gap_report(record(hand_table()))
    lines = driver.format_domain_gap_report(gap, top=5).split("\n")
    assert len(lines) == 4 and lines[0].split() == ["layer", "kind", "gap", "gap_max", "channel", "mean_shift", "dead_a", "dead_b", "dead_ab"]
    assert lines[1].split()[0] == "input" and lines[2].split() == ["conv", "conv", "{:.3e}".format(gap["layers"][1]["gap"]),
                                                                   "{:.3e}".format(gap["layers"][1]["gap_max"]), "0",
                                                                   "{:.3e}".format(gap["layers"][1]["mean_shift"]), "1", "0", "1"]
    assert len(lines[0]) == len(lines[1]) == len(lines[2]) and lines[3] == "backbone: 2 layers; largest gap: input"
    assert len(driver.format_domain_gap_report(gap, top=1).split("\n")) == 3


def test_plan_layout_and_prefixes_for_mixed_shapes():
    from dasac_hip import ops
    plan = ops.ActivationStatsPlan([(3, 65, 65), (64, 33, 33), (1, 7), (19, 9, 9)], 5, (2,))
    assert plan.bounds == (0, 2, 5) and plan.N == 5
    assert plan.shapes == ((3, 4225), (64, 1089), (1, 7), (19, 81))
    assert plan.row0 == [0, 3, 67, 68] and plan.plane0 == [0, 15, 335, 340] and plan.R == 87 and plan.n_planes == 435
    assert plan.bytes_read == 4.0 * 5 * (3 * 4225 + 64 * 1089 + 7 + 19 * 81)
    assert plan.rows.dtype.itemsize == 32 and plan.rows.tobytes() == b"".join(
        np.asarray([0, hw], dtype="<i8").tobytes() + np.asarray([c, r0], dtype="<i4").tobytes() + np.asarray([p0], dtype="<i8").tobytes()
        for (c, hw), r0, p0 in zip(plan.shapes, plan.row0, plan.plane0))
    assert ops.activation_stats_plan([(3, 65, 65)], 2, None) is ops.activation_stats_plan(((3, 65, 65),), 2, (0, 2))
    assert ops.activation_stats_plan([(3, 65, 65)], 2, (1,)) is not ops.activation_stats_plan([(3, 65, 65)], 2, None)
    assert ops.ACTIVATION_STATS_COLUMNS == ref.COLUMNS


def test_python_layer_refuses_bad_bounds_shapes_and_cpu_tensors():
    from dasac_hip import ops, DasacError
    assert ops.segment_bounds(None, 4) == (0, 4) and ops.segment_bounds((1,), 4) == (0, 1, 4) and ops.segment_bounds((0, 2, 3, 4), 4) == (0, 2, 3, 4)
    assert ops.segment_bounds([2, 3], 5) == (0, 2, 3, 5)
    for bad, n in [((0, 3, 2, 5), 5), ((0, 2, 4), 5), ((0, 2, 2, 5), 5), ((5,), 5), ((0,), 5), ((3, 1), 5), (tuple(range(10)), 9), (None, 0)]:
        with pytest.raises(DasacError):
            ops.segment_bounds(bad, n)
        with pytest.raises(DasacError):
            ops.ActivationStatsPlan([(2, 3, 3)], n, bad)
    assert ops.segment_bounds(tuple(range(9)), 8) == tuple(range(9))      # eight segments of one sample: the most there are
    for shapes in ([], [(0, 3, 3)], [(2, 0, 3)]):
        with pytest.raises(DasacError):
            ops.ActivationStatsPlan(shapes, 2)
    plan = ops.ActivationStatsPlan([(2, 3, 3)], 2)
    with pytest.raises(DasacError):
        plan.run([torch.zeros(2, 2, 3, 3)])                   # no CPU path


def test_engine_layout_names_are_unique_and_follow_named_modules():
    import models
    import torch.nn as nn
    from types import SimpleNamespace as NS
    from oracle.step_ref import DEFAULT_CFG
    from dasac_hip import engine as E
    cfg = NS(**dict(DEFAULT_CFG, INIT_MODEL="", OPT_NESTEROV=False))
    net = models.get_model(cfg, 0, num_classes=19, criterion=nn.CrossEntropyLoss(ignore_index=255, reduction="none"))
    eng = E.Engine(net.backbone._plan())
    assert eng.probe is None
    shapes, (c, h, w) = [(3, 65, 65)], (3, 65, 65)
    for op in eng.plan.ops:                                   # a straight walk gives every op SOME shape: only names matter here
        shapes.append(op.tensors(c, h, w)[-1])
    names = {m: name for name, m in net.backbone.named_modules()}
    layout = eng.activation_layout(shapes, names)
    assert len(layout) == len(eng.plan.ops) + 1 and layout[0]["name"] == "input" and layout[0]["op"] == -1 and layout[0]["slot"] == 0
    assert len(set(e["name"] for e in layout)) == len(layout)
    assert [e["op"] for e in layout[1:]] == list(range(len(eng.plan.ops))) and [e["slot"] for e in layout[1:]] == [op.dst for op in eng.plan.ops]
    assert layout[1]["name"] == "model.conv1" and layout[1]["relu"] and layout[2]["name"] == "pool@2" and layout[2]["kind"] == "pool"
    assert layout[-1]["name"] == "model.layer5.conv2d_list" and layout[-1]["C"] == 19 and not layout[-1]["relu"]      # the four ASPP branches
    assert [e["row0"] for e in layout] == list(np.cumsum([0] + [e["C"] for e in layout[:-1]]))
    bare = eng.activation_layout(shapes)                      # without names every conv falls back to its slot
    assert bare[1]["name"] == "conv@1" and len(set(e["name"] for e in bare)) == len(bare)


def test_activation_probe_attaches_to_both_engines_and_detaches():
    import driver
    import models
    import torch.nn as nn
    from types import SimpleNamespace as NS
    from oracle.step_ref import DEFAULT_CFG
    cfg = NS(**dict(DEFAULT_CFG, INIT_MODEL="", OPT_NESTEROV=False))
    net = models.get_model(cfg, 0, num_classes=19, criterion=nn.CrossEntropyLoss(ignore_index=255, reduction="none"))
    wrapped = NS(module=net)                                  # what a DistributedDataParallel wrapper looks like from outside
    with driver.activation_probe(wrapped, bounds=(2,)) as probe:
        taps = net.backbone._engine.probe, net.slow_net._engine.probe
        assert (taps[0].net, taps[1].net) == ("backbone", "slow_net") and taps[0].bounds == (2,) and probe.passes == []
        assert taps[0].names[net.backbone.model.conv1] == "model.conv1"
        with pytest.raises(RuntimeError):                     # one probe at a time
            with driver.activation_probe(net):
                pass
        assert net.backbone._engine.probe is taps[0] and net.slow_net._engine.probe is taps[1]
        taps[1].append(("table", [], 3, (0, 3)))
        assert [(r.net, r.N, r.bounds, r.table) for r in probe.passes] == [("slow_net", 3, (0, 3), "table")]
    assert net.backbone._engine.probe is None and net.slow_net._engine.probe is None


def test_bad_arguments_are_refused_on_the_host():
    """The entry point validates before it launches (no device needed for a refusal)."""
    from dasac_hip import lib as L
    lib = L.load()
    assert L.PROTOTYPES["dasac_activation_stats_workspace"] == (ctypes.c_size_t, [ctypes.c_int64])
    assert len(L.PROTOTYPES["dasac_activation_stats"][1]) == 10
    ws = lib.dasac_activation_stats_workspace
    assert ws(0) == 0 and ws(-3) == 0 and ws(1) == 48 and ws(3 * 10 ** 9) == 144 * 10 ** 9
    buf = (ctypes.c_double * 16)()
    at = ctypes.addressof(buf)
    call = lambda *a: lib.dasac_activation_stats(*a, None)
    #            tensors n_t N  R  seg n_seg ws bytes table
    assert call(None, 1, 1, 1, at, 1, at, 48, at) != 0 and b"null" in lib.dasac_last_error()
    assert call(at, 1, 1, 1, None, 1, at, 48, at) != 0 and call(at, 1, 1, 1, at, 1, None, 48, at) != 0 and call(at, 1, 1, 1, at, 1, at, 48, None) != 0
    assert call(at, 0, 1, 1, at, 1, at, 48, at) != 0 and b"tensors" in lib.dasac_last_error()
    assert call(at, 1, 0, 1, at, 1, at, 48, at) != 0 and b"N >= 1" in lib.dasac_last_error()
    assert call(at, 2, 1, 1, at, 1, at, 48, at) != 0                                            # fewer channel rows than tensors
    assert call(at, 1, 1, 1, at, 0, at, 48, at) != 0 and b"segments" in lib.dasac_last_error()
    assert call(at, 1, 9, 1, at, 9, at, 9 * 48, at) != 0 and call(at, 1, 2, 1, at, 3, at, 96, at) != 0      # > 8, and more segments than samples
    assert call(at, 1, 2, 3, at, 1, at, 6 * 48 - 1, at) != 0 and b"workspace" in lib.dasac_last_error()
    assert call(at, 1, 1 << 20, 1 << 12, at, 1, at, 1 << 60, at) != 0 and b"planes" in lib.dasac_last_error()
    assert call(at, 1, 1, 1, at, 1, at, 48, at + 4) != 0 and b"misaligned" in lib.dasac_last_error()
    assert not any(buf)
