"""Label-free view consistency -- the parts that need no GPU: the host summary and report of driver.py on tables worked out by
hand, the rule that says which rank counts a group whose views are spread over ranks, the numpy reference on a pixel worked out
by hand, and the refusals that must come before any device work."""
import numpy as np
import pytest
import torch

from consistency_ref import lattice, view_consistency_ref

NAMES = ["road", "car", "sky"]


def _tables(C, T):
    return {"agree": torch.zeros(C + 1, T + 1, T + 1, dtype=torch.int64), "flips": torch.zeros(C, C, dtype=torch.int64),
            "per_view": torch.zeros(T, 2, dtype=torch.int64)}


def _hand_tables():
    """C = 3, T = 3.  road: 60 pixels at k=3,m=3, 20 at k=3,m=2, 20 at k=2,m=2, 7 at k=1 (counted nowhere); car: 10 at k=2,m=1;
    sky: k=1 pixels only; 5 pixels uncovered."""
    t = _tables(3, 3)
    A = t["agree"]
    A[0, 3, 3], A[0, 3, 2], A[0, 2, 2], A[0, 1, 1] = 60, 20, 20, 7
    A[1, 2, 1] = 10
    A[2, 1, 1], A[2, 1, 0] = 4, 4
    A[3, 0, 0] = 5
    F = t["flips"]
    F[0, 0] = 60 * 3 + 20 * 1 + 20 * 1          # agreeing pairs on road
    F[0, 1], F[1, 0] = 25, 15                    # road <-> car, either order: 40 pairs
    F[1, 2] = 10                                 # car <-> sky
    t["per_view"][:] = torch.tensor([[130, 120], [100, 90], [60, 50]])
    return t


def test_summarise_consistency_on_a_hand_written_table():
    import driver
    s = driver.summarise_consistency(_hand_tables())
    road, car, sky = s["classes"]
    assert road["pixels"] == 100 and car["pixels"] == 10 and sky["pixels"] == 0
    assert road["agreement"] == pytest.approx((60 * 3 + 20 * 2 + 20 * 2) / (80 * 3 + 20 * 2), abs=1e-12)
    assert road["unanimous"] == pytest.approx(0.8, abs=1e-12) and road["by_k"] == pytest.approx([0, 0, 0.2, 0.8], abs=1e-12)
    assert car["agreement"] == pytest.approx(0.5, abs=1e-12) and car["unanimous"] == 0.0 and car["by_k"] == [0, 0, 1.0, 0]
    assert sky == dict(pixels=0, agreement=0.0, unanimous=0.0, by_k=[0.0] * 4)           # k = 1 pixels cannot disagree
    assert s["agreement"] == pytest.approx((100 * road["agreement"] + 10 * 0.5) / 110, abs=1e-12)
    assert s["class_mean_agreement"] == pytest.approx((road["agreement"] + 0.5) / 2, abs=1e-12)
    assert s["classes_present"] == 2
    assert s["uncovered_share"] == pytest.approx(5 / 130, abs=1e-12)
    assert [(f["a"], f["b"], f["pairs"]) for f in s["flips"]] == [(0, 1, 40), (1, 2, 10)]
    assert s["flips"][0]["share_a"] == pytest.approx(40 / 260, abs=1e-12) and s["flips"][0]["share_b"] == pytest.approx(40 / 50, abs=1e-12)
    assert s["flips"][1]["share_b"] == pytest.approx(1.0, abs=1e-12)
    assert [v["coverage"] for v in s["views"]] == pytest.approx([1.0, 100 / 130, 60 / 130], abs=1e-12)
    assert [v["agreement"] for v in s["views"]] == pytest.approx([120 / 130, 0.9, 50 / 60], abs=1e-12)
    assert len(driver.summarise_consistency(_hand_tables(), top=1)["flips"]) == 1


def test_summarise_consistency_leaves_ignored_classes_out_of_the_scores():
    import driver
    s = driver.summarise_consistency(_hand_tables(), ignore_classes=[1])
    assert s["agreement"] == pytest.approx(s["classes"][0]["agreement"], abs=1e-12) == pytest.approx(s["class_mean_agreement"], abs=1e-12)
    assert s["classes_present"] == 1 and s["flips"] == []                              # both flips involve car
    assert s["classes"][1]["pixels"] == 10                                             # still reported per class


def test_summarise_consistency_all_uncovered_and_collapsed():
    import driver
    t = _tables(3, 2)
    t["agree"][3, 0, 0] = 50
    s = driver.summarise_consistency(t)
    assert s["agreement"] == 0.0 and s["class_mean_agreement"] == 0.0 and s["classes_present"] == 0 and s["uncovered_share"] == 1.0
    assert s["flips"] == [] and all(v == dict(coverage=0.0, agreement=0.0) for v in s["views"])
    # a collapsed model: one class everywhere, every view agrees -- the score is 1.0, and classes_present says why
    t = _tables(3, 2)
    t["agree"][1, 2, 2], t["flips"][1, 1] = 1000, 1000
    t["per_view"][:] = 1000
    s = driver.summarise_consistency(t)
    assert s["agreement"] == 1.0 and s["class_mean_agreement"] == 1.0 and s["classes_present"] == 1 and s["flips"] == []
    assert "collapsed" in driver.summarise_consistency.__doc__.lower() and "1.0" in driver.summarise_consistency.__doc__
    # one view: no pixel has k >= 2
    t = _tables(2, 1)
    t["agree"][0, 1, 1], t["per_view"][0, 0], t["per_view"][0, 1] = 9, 9, 9
    s = driver.summarise_consistency(t)
    assert s["agreement"] == 0.0 and s["classes_present"] == 0 and s["views"] == [dict(coverage=1.0, agreement=1.0)]


def test_format_consistency_renders_every_class_flip_and_view():
    import driver
    s = driver.summarise_consistency(_hand_tables())
    text = driver.format_consistency(s, NAMES)
    lines = text.split("\n")
    assert "2 of 3 classes present" in lines[0] and "{:.4f}".format(s["agreement"]) in lines[0]
    assert lines[1].split() == ["class", "pixels", "agree", "unanim", "k=2", "k=3"]
    assert lines[2].split() == ["road", "100", "{:.4f}".format(s["classes"][0]["agreement"]), "0.8000", "0.200", "0.800"]
    assert lines[4].split()[:2] == ["sky", "0"]
    assert "road <-> car 40" in lines[5] and "car <-> sky 10" in lines[5]
    assert lines[6].startswith("views: 0: covers 1.0000") and len(lines) == 7
    with pytest.raises(AssertionError):
        driver.format_consistency(s, NAMES[:2])


@pytest.mark.parametrize("world", [2, 4, 8])
@pytest.mark.parametrize("T", [2, 4])
def test_consistency_owner_counts_every_group_once(world, T):
    """Per-rank batches B as `prep_batch` deals them: whole groups (B a multiple of T: every rank counts its own), or a group spread
    over T // B consecutive ranks, each of which holds the gathered group (`SAC._gather`) -- exactly one of them may count it."""
    from models.sac import consistency_owner
    for B in [b for b in (1, 2, 4, 8) if (b >= T and b % T == 0) or (b < T and T % b == 0 and (world * b) % T == 0)]:
        counted = {}
        for rank in range(world):
            if B >= T:
                groups = [(rank, g) for g in range(B // T)]             # its own groups, nobody else's
            else:
                groups = [("shared", (rank * B) // T)]                  # the group its views belong to (driver.prep_batch)
            if consistency_owner(rank, B, T):
                for g in groups:
                    counted[g] = counted.get(g, 0) + 1
            else:
                assert B < T
        assert sorted(counted.values()) == [1] * (world * B // T), (world, T, B, counted)


def test_reference_on_a_pixel_worked_out_by_hand():
    """T = 3, C = 3, two pixels.  Pixel 0: views 0 and 1 covered (labels 2 and 0), view 2 a rim weight of 1/4 on class 0 -- the
    consensus is class 0 through the rim weight, k = 2, m = 1.  Pixel 1: nothing covered."""
    a = np.zeros((3, 3, 1, 2), np.float32)
    a[0, :, 0, 0] = [0.25, 0.25, 0.5]
    a[1, :, 0, 0] = [0.5, 0.25, 0.25]
    a[2, :, 0, 0] = [0.25, 0, 0]
    a[1, :, 0, 1] = [0.25, 0, 0]
    agree, flips, per_view = view_consistency_ref(a, 3)
    want = np.zeros((4, 4, 4), np.int64)
    want[0, 2, 1], want[3, 0, 0] = 1, 1
    assert np.array_equal(agree, want)
    assert flips.sum() == 1 and flips[2, 0] == 1                                       # view 0 says 2, view 1 says 0
    assert per_view.tolist() == [[1, 0], [1, 1], [0, 0]]
    agree, flips, per_view = view_consistency_ref(a, 3, cover=0.2)                      # the rim weights now count as covered
    want[:] = 0
    want[0, 3, 2], want[0, 1, 1] = 1, 1
    assert np.array_equal(agree, want) and flips[2, 0] == 2 and flips[0, 0] == 1 and flips.sum() == 3


def test_lattice_is_exactly_summable():
    rng = np.random.default_rng(0)
    a = lattice(rng, 2, 4, 19, 5, 7)
    assert a.dtype == np.float32 and a.shape == (8, 19, 5, 7)
    q = a.astype(np.float64) * 4096
    assert np.array_equal(q, np.round(q)) and set(np.unique(q.sum(1))) <= {0.0, 1024.0, 3072.0, 4096.0}
    labels = rng.integers(0, 19, (2, 4, 5, 7))
    b = lattice(rng, 2, 4, 19, 5, 7, labels=labels, coverage=np.full((2, 4, 5, 7), 4))
    assert np.array_equal(b.argmax(1).reshape(2, 4, 5, 7), labels) and (b.sum(1) == 1).all()


def test_view_consistency_refuses_cpu_tensors():
    from dasac_hip import ops, DasacError
    with pytest.raises(DasacError):
        ops.view_consistency(torch.rand(4, 19, 4, 4), 2)


def test_consistency_tables_are_views_of_one_buffer():
    from dasac_hip import ops, DasacError
    t = ops.consistency_tables(19, 4, "cpu")
    assert t.buffer.numel() == 20 * 25 + 361 + 8 == ops.consistency_size(19, 4) and t.buffer.dtype == torch.int64
    assert tuple(t.agree.shape) == (20, 5, 5) and tuple(t.flips.shape) == (19, 19) and tuple(t.per_view.shape) == (4, 2)
    t.agree[19, 0, 0], t.flips[0, 0], t.per_view[3, 1] = 1, 2, 3
    assert t.buffer[19 * 25] == 1 and t.buffer[500] == 2 and t.buffer[-1] == 3 and int(t.buffer.sum()) == 6
    agree, flips, per_view = t
    assert agree is t.agree and flips is t.flips and per_view is t.per_view
    with pytest.raises(DasacError):
        ops.ConsistencyTables(torch.zeros(10, dtype=torch.int64), 19, 4)
    with pytest.raises(DasacError):
        ops.ConsistencyTables(torch.zeros(2 * ops.consistency_size(19, 4), dtype=torch.int64)[::2], 19, 4)


def test_validation_refuses_consistency_on_the_source_step_before_it_touches_the_loader():
    import driver

    class Loader:
        def __iter__(self):
            raise AssertionError("the loader was touched")

        def __len__(self):
            raise AssertionError("the loader was touched")
    with pytest.raises(ValueError):
        driver.validation(torch.nn.Linear(1, 1), Loader(), step="source", consistency=True)
    with pytest.raises(ValueError):                                                     # a net without the hook
        driver.validation(torch.nn.Linear(1, 1), Loader(), step="target", group_size=2, consistency=True)
