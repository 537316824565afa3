"""Pins the host-side report readers byte for byte: the exact text of every `format_*` and a canonical dump of every
`summarise_*` / `*_report` / helper result (floats as float.hex(), tensors and arrays as nested lists with their dtype, dict
keys sorted, NaN and inf spelled out) against tests/golden/report_texts.json.  The inputs are small hand-written or seeded tables
built here, on the CPU.  The fixture holds recorded results only; it was recorded from the driver.py that preceded the split
into reports.py (`python tests/test_reports_pinned_cpu.py --record`) and is compared with no tolerance."""
import json
import math
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "report_texts.json")
NAMES = ["road", "sidewalk", "pole"]                        # 3 classes


def canon(v):
    if isinstance(v, (bool, str)) or v is None:
        return v
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, (float, np.floating)):
        v = float(v)
        return "nan" if math.isnan(v) else ("inf" if v == math.inf else ("-inf" if v == -math.inf else v.hex()))
    if isinstance(v, torch.Tensor):
        return {"dtype": str(v.dtype), "data": canon(v.tolist())}
    if isinstance(v, np.ndarray):
        return {"dtype": str(v.dtype), "data": canon(v.tolist())}
    if isinstance(v, NS):
        return canon(vars(v))
    if isinstance(v, dict):
        return {str(k): canon(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [canon(x) for x in v]
    raise TypeError(type(v))


# ------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------
def _matrix():
    # row = ground truth, column = prediction, index 3 = no class; class 2 never occurs in the ground truth; 3 appears twice off
    # the diagonal (ties by index)
    return torch.tensor([[50, 3, 0, 2], [4, 30, 0, 1], [0, 0, 0, 0], [5, 3, 1, 7]], dtype=torch.int64)


def _teacher_matrix():
    return torch.tensor([[52, 4, 1, 0], [6, 28, 1, 0], [0, 0, 0, 0], [7, 2, 2, 0]], dtype=torch.int64)


def _boundary_tables():
    rs = np.random.RandomState(3)
    T = rs.randint(0, 40, size=(3, 5, 3)).astype(np.int64)          # R = 2: [R+1, 5, C]
    T[:, :, 2] = 0                                                  # class 2 has no pixel
    T[:, 4] = np.minimum(T[:, 4], T[:, 3])
    U = rs.randint(0, 9, size=(3, 5, 3)).astype(np.int64)
    return {"logits_up": torch.from_numpy(T), "teacher_labels": torch.from_numpy(U), "empty": torch.zeros(3, 5, 3, dtype=torch.int64)}


def _consistency_tables():
    rs = np.random.RandomState(5)
    A = np.zeros((4, 4, 4), np.int64)                               # agree[c*][k][m], C = 3, T = 3
    for c in (0, 2):                                                # class 1 has no pixel seen by two views
        for k in range(1, 4):
            for m in range(1, k + 1):
                A[c, k, m] = rs.randint(0, 60)
    A[1, 1, 1] = 9
    A[3, 0, 0] = 17
    F = np.array([[40, 6, 6], [2, 0, 1], [3, 0, 25]], np.int64)     # S[0,1] == 8, S[0,2] == 9, S[1,2] == 1
    V = np.array([[120, 100], [80, 33], [0, 0]], np.int64)          # view 2 covers nothing
    return {"agree": torch.from_numpy(A), "flips": torch.from_numpy(F), "per_view": torch.from_numpy(V)}


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(3, 2)
        self.b = torch.nn.Linear(1, 4)


def _optim(net):
    table = torch.tensor([[4.0, 1.5, 0, 0, 1, 9.0, 2.0, 0.25],       # TENSOR_STATS_COLUMNS
                          [0.25, 0.5, 2, 2, 0, 1.0, 1.0, 0.0],       # a.bias: two non-finite entries, the first at index 1
                          [0, 0, 0, 0, 0, 0, 0, 0],                  # b.weight: no pending gradient, zero weights
                          [12.0, 3.0, 0, 0, 0, 16.0, 4.0, 1.0]], dtype=torch.float64)
    groups = [dict(params=[net.a.weight, net.a.bias], lr=0.01), dict(params=[net.b.weight, net.b.bias], lr=0.1)]
    return NS(param_groups=groups, tensor_stats=table, last_skipped_stats=(table * 0.5, torch.tensor(3)))


def _activation_record(seed, net="backbone"):
    """3 layers, N = 3 samples in 2 segments, statistics computed from exactly summable activations (multiples of 1/4)."""
    rs = np.random.RandomState(seed)
    layout = [dict(name="conv1", kind="conv", C=2, H=2, W=2, row0=0), dict(name="layer1.relu", kind="relu", C=3, H=2, W=2, row0=2),
              dict(name="fc", kind="conv", C=2, H=1, W=1, row0=5)]
    bounds, N = (0, 2, 3), 3
    table = np.zeros((2, 7, 6))
    for e in layout:
        x = rs.randint(-8, 9, size=(N, e["C"], e["H"], e["W"])) / 4.0
        if e["kind"] == "relu":
            x = np.maximum(x, 0.0)
            x[:, 1] = 0.0                                           # a dead channel in both segments
            x[:2, 2] = 0.0                                          # and one dead in segment 0 only
        if e["name"] == "fc":
            x[1, 1, 0, 0] = np.nan                                  # the non-finite layer (segment 0)
        for s in range(2):
            for c in range(e["C"]):
                v = x[bounds[s]:bounds[s + 1], c]
                ok = np.isfinite(v)
                bad = [i for i in range(x.size) if not np.isfinite(x.flat[i]) and np.unravel_index(i, x.shape)[1] == c
                       and bounds[s] <= np.unravel_index(i, x.shape)[0] < bounds[s + 1]]
                table[s, e["row0"] + c] = [v[ok].sum(), (v[ok] ** 2).sum(), np.abs(v[ok]).max() if ok.any() else 0.0, (~ok).sum(),
                                           bad[0] + 1 if bad else 0, (v == 0).sum()]
    return NS(net=net, N=N, bounds=bounds, table=torch.from_numpy(table), layout=layout)


def _class_table(seed, counts, Cf=4, like=None):
    rs = np.random.RandomState(seed)
    n = np.asarray(counts, np.int64)
    mu = rs.randint(-8, 9, size=(len(n), Cf)) / 4.0
    var = rs.randint(1, 9, size=(len(n), Cf)) / 8.0
    sums = np.stack([mu * n[:, None], (var + mu ** 2) * n[:, None]], -1)
    sums[:, 3] = 0.0                                                # feature 3 is dead in every class
    if like is not None:
        sums[0], n[0] = like.sums[0].numpy(), like.counts[0]        # class 0 did not move: gap 0
    return NS(sums=torch.from_numpy(sums), counts=torch.from_numpy(n))


# ------------------------------------------------------------------------------------------------------------------
# the calls, one function per family: {key: canonical result}
# ------------------------------------------------------------------------------------------------------------------
def _iou(d):
    counts = torch.tensor([[50, 30, 0], [9, 6, 1], [5, 5, 0]], dtype=torch.int64)
    other = torch.tensor([[41, 0, 3], [2, 0, 8], [7, 11, 1]], dtype=torch.int64)
    return {"summarise_iou": d.summarise_iou(counts),
            "summarise_validation": d.summarise_validation({"logits_up": counts, "teacher_labels": other}),
            "summarise_validation/ignore": d.summarise_validation({"logits_up": counts, "teacher_labels": other}, ignore_classes=(2,)),
            "stat_mean": [d.stat_mean([0.5, 0.25, 1.0]), d.stat_mean([]), d.stat_mean([1.0, -1.0]), d.stat_mean([0.1, 0.2, 0.3])],
            "class_subset_mean": [d.class_subset_mean(torch.tensor([0.5, 0.25, 0.1])), d.class_subset_mean([0.5, 0.25, 0.1], (1,)),
                                  d.class_subset_mean(np.array([0.3, 0.7, 0.9]), ignore_classes=(0, 2))]}


def _confusion(d):
    M, Mt = _matrix(), _teacher_matrix()
    table = torch.tensor([[[3, 1], [0, 0], [2, 6], [1, 20]], [[0, 0], [0, 0], [0, 0], [0, 0]], [[4, 0], [2, 2], [0, 5], [0, 9]]],
                         dtype=torch.int64)                         # [C, 4 bins, miss / hit]: an empty bin, an empty class
    return {"counts_from_confusion": d.counts_from_confusion(M),
            "counts_from_confusion/layers": d.counts_from_confusion(torch.stack([M, Mt])),
            "summarise_confusion": d.summarise_confusion(M),
            "summarise_confusion/ignore_top": d.summarise_confusion(M, ignore_classes=(1,), top=2),
            "summarise_confusion/top1": d.summarise_confusion(Mt, top=1),
            "pseudo_label_audit": d.pseudo_label_audit(M, Mt),
            "summarise_reliability": d.summarise_reliability(table),
            "format_confusion": d.format_confusion(M, NAMES),
            "format_confusion/wide": d.format_confusion(M * 123457, ["a", "a-long-class-name", "c"])}


def _boundary(d):
    tables = _boundary_tables()
    full = d.summarise_boundary(tables, radii=(1, 2))
    ignore = d.summarise_boundary({"logits_up": tables["logits_up"]}, ignore_classes=(0,), radii=(2,))
    return {"summarise_boundary": full, "summarise_boundary/ignore": ignore,
            "format_boundary": d.format_boundary(full, NAMES), "format_boundary/ignore": d.format_boundary(ignore, NAMES)}


def _consistency(d):
    tables = _consistency_tables()
    full = d.summarise_consistency(tables)
    small = d.summarise_consistency(NS(**tables), ignore_classes=(2,), top=1)
    top1 = d.summarise_consistency(tables, top=1)
    empty = d.summarise_consistency({k: torch.zeros_like(v) for k, v in tables.items()})
    return {"summarise_consistency": full, "summarise_consistency/ignore_top": small, "summarise_consistency/top1": top1,
            "summarise_consistency/empty": empty, "format_consistency": d.format_consistency(full, NAMES),
            "format_consistency/ignore_top": d.format_consistency(small, NAMES),
            "format_consistency/empty": d.format_consistency(empty, NAMES)}


def _gradient(d):
    net = _Net()
    optim = _optim(net)
    wrapped = NS(module=net)
    full = d.gradient_report(net, optim)
    top2 = d.gradient_report(wrapped, optim, top=2)
    zeros = d.gradient_report(net, optim, table=torch.zeros(4, 8, dtype=torch.float64))
    skipped = d.skipped_step_report(net, optim, top=1)
    return {"gradient_report": full, "gradient_report/top2": top2, "gradient_report/zeros": zeros, "skipped_step_report": skipped,
            "format_gradient_report": d.format_gradient_report(full), "format_gradient_report/top2": d.format_gradient_report(top2, top=2),
            "format_gradient_report/top0": d.format_gradient_report(full, top=0),
            "format_gradient_report/zeros": d.format_gradient_report(zeros, top=1),
            "format_gradient_report/skipped": d.format_gradient_report(skipped, top=1)}


def _activation(d):
    a, b = _activation_record(7), _activation_record(11)
    seg0, seg1 = d.activation_report(a), d.activation_report(a, segment=1, top=2)
    one, two = d.domain_gap_report(a), d.domain_gap_report(a, b, top=2)
    mu, var = np.array([0.5, 0.0, -1.25, 0.0]), np.array([0.25, 0.0, 2.0, 0.0])
    return {"activation_report": seg0, "activation_report/segment1_top2": seg1, "domain_gap_report": one, "domain_gap_report/two": two,
            "moment_gap": d.moment_gap(mu, var, np.array([0.25, 0.0, -1.25, 1e-20]), np.array([1.0, 0.0, 2.0, 0.0])),
            "format_activation_report": d.format_activation_report(seg0), "format_activation_report/top1": d.format_activation_report(seg0, top=1),
            "format_activation_report/segment1": d.format_activation_report(seg1, top=2),
            "format_domain_gap_report": d.format_domain_gap_report(one), "format_domain_gap_report/top2": d.format_domain_gap_report(two, top=2),
            "format_domain_gap_report/top0": d.format_domain_gap_report(two, top=0)}


def _class_gap(d):
    a = _class_table(13, [40, 0, 5])                                # class 1 absent, class 2 under min_nodes = 16
    b = _class_table(17, [32, 20, 18])
    same = _class_table(19, [32, 20, 18], like=a)
    rec_a, rec_b = NS(table=a, layer="layer4"), NS(table=b, layer="layer4")
    calls = {"class_gap_report": d.class_gap_report(rec_a, rec_b), "class_gap_report/min4": d.class_gap_report(a, b, min_nodes=4),
             "class_gap_report/within": d.class_gap_report(rec_b, min_nodes=4, top=2),
             "class_gap_report/ignore": d.class_gap_report(b, same, ignore_classes=(1,), min_nodes=4),
             "class_gap_report/same": d.class_gap_report(a, same, min_nodes=4, top=1)}
    out = dict(calls)
    for key, report in calls.items():
        out["format_" + key] = d.format_class_gap_report(report, None if key.endswith("min4") else NAMES)
    return out


FAMILIES = {"iou": _iou, "confusion": _confusion, "boundary": _boundary, "consistency": _consistency, "gradient": _gradient,
            "activation": _activation, "class_gap": _class_gap}


def run_family(family):
    import driver
    return {key: json.dumps(canon(value), sort_keys=True) for key, value in FAMILIES[family](driver).items()}


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_report_readers_reproduce_the_recorded_results(family, recorded):
    got, want = run_family(family), recorded[family]
    assert sorted(got) == sorted(want)
    for key in sorted(got):
        assert got[key] == json.dumps(want[key], sort_keys=True), key


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], "usage: python tests/test_reports_pinned_cpu.py --record"
    sys.path.insert(0, os.path.join(ROOT, "da-sac_amd"))
    blob = {family: {key: json.loads(text) for key, text in run_family(family).items()} for family in sorted(FAMILIES)}
    with open(FIXTURE, "w") as f:
        json.dump(blob, f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print("recorded", sum(len(v) for v in blob.values()), "results,", os.path.getsize(FIXTURE), "bytes")
