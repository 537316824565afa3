"""The per-tensor gradient health table of the fused optimisers (`track_tensor_stats`, dasac_tensor_stats): `optim.tensor_stats`,
`optim.last_skipped_stats`, `optim.measure_tensor_stats()` and `driver.gradient_report`.

Shapes: those of tests/test_gpu_fused_optim.py (1 element; 4097 = one chunk + 1; 19x2048x3x3 = 85.5 chunks; an all-zero gradient;
a parameter whose first gradient comes a step late).  All four kinds of update, with and without a stash.

Reference and tolerances.  The reference is torch float64 on d = g2 + g formed in fp32, on p and on the state as they stand
before the step.  Columns 1-4 and 6 (maxima, counts, the first index) must be EQUAL.  Columns 0, 5 and 7 are sums of n
non-negative products that are exact in double, added in double on both sides: any summation order is within (n - 1) * 2^-53
relative of the exact sum, so two orders differ by at most 2 * n * 2^-53 relative, n = the tensor's numel.  Everything else
(placement, repeats, capture, read-only) is torch.equal."""
import numpy as np
import pytest
import torch

from test_gpu_fused_optim import LATE, SHAPES, ZERO, make_params, rn101_state, sac_net, three_groups  # noqa: F401
from test_gpu_grad_clip import KINDS, STATE, all_state, draw, fused, offset_view, summed

pytestmark = pytest.mark.gpu

BIG, ONE = 3, 4               # (19, 2048, 3, 3): 85.5 chunks; (1,)
COLS = 8
EXACT, SUMS = (1, 2, 3, 4, 6), (0, 5, 7)


def hand_over(opt, ps, g1, g2, stash, place=False):
    """The fused side of driver.sac_train_iteration.  stash: g1 is the first pass (stashed; parameter 0 takes no part in it), g2
    the second (parameter 1 takes no part).  Without: g1 alone in .grad.  place: BIG's gradients as views 4 bytes into a flat buffer.
    Returns the gradient each parameter's update applies, as fp32 host tensors (None: nothing pending)."""
    def give(grads):
        for i, (p, gr) in enumerate(zip(ps, grads)):
            t = None if gr is None else gr.cuda()
            p.grad = offset_view(t) if t is not None and place and i == BIG else t
    opt.zero_grad()
    if not stash:
        give(g1)
        return list(g1)
    give([None if i == 0 else gr for i, gr in enumerate(g1)])
    opt.stash_grads()
    give([None if i == 1 else gr for i, gr in enumerate(g2)])
    return summed(g1, g2)


def reference(ps, applied, states):
    """fp64 [n, 8] on the host from the fp32 gradients the update applies, the parameters and the states (None: absent)."""
    out = torch.zeros(len(ps), COLS, dtype=torch.float64)
    for i, (p, d, s) in enumerate(zip(ps, applied, states)):
        if d is None:
            continue
        d = d.detach().cpu().reshape(-1).to(torch.float64)
        w = p.detach().cpu().reshape(-1).to(torch.float64)
        fin, wfin = torch.isfinite(d), torch.isfinite(w)
        bad = torch.nonzero(~fin)
        out[i, 0] = (d[fin] * d[fin]).sum()
        out[i, 1] = d[fin].abs().max() if bool(fin.any()) else 0.0
        out[i, 2] = int((~fin).sum())
        out[i, 3] = int(bad[0]) + 1 if len(bad) else 0
        out[i, 4] = int((d == 0).sum())
        out[i, 5] = (w * w).sum()
        out[i, 6] = w[wfin].abs().max() if bool(wfin.any()) else 0.0
        if s is not None:
            s = s.detach().cpu().reshape(-1).to(torch.float64)
            out[i, 7] = (s * s).sum()
    return out


def assert_matches(table, ref, ps, tag=""):
    assert table.dtype == torch.float64 and table.is_cuda and tuple(table.shape) == (len(ps), COLS)
    t = table.cpu()
    for i, p in enumerate(ps):
        for c in EXACT:
            assert float(t[i, c]) == float(ref[i, c]), (tag, i, c, float(t[i, c]), float(ref[i, c]))
        bound = 2.0 * p.numel() * 2.0 ** -53
        for c in SUMS:
            a, b = float(t[i, c]), float(ref[i, c])
            print("{} tensor {} col {}: {:.17e} vs fp64 {:.17e} (rel {:.2e}, bound {:.2e})".format(tag, i, c, a, b, abs(a - b) / b if b else 0.0, bound))
            assert abs(a - b) <= bound * b, (tag, i, c, a, b)


def states_of(opt, ps, kind):
    """The state tensor the table reports (momentum_buffer / exp_avg) as it stands, None where there is none yet."""
    return [None if opt.state.get(p, {}).get(STATE[kind][0]) is None else opt.state[p][STATE[kind][0]].detach().clone() for p in ps]


def within_one_ulp(a, b):
    """fp32 0-dim tensors: a is b or one of b's two neighbours."""
    lo, hi = torch.nextafter(b, torch.full_like(b, -float("inf"))), torch.nextafter(b, torch.full_like(b, float("inf")))
    return bool((a >= lo) & (a <= hi))


def norm_of(table):
    return torch.sqrt(table[:, 0].sum()).to(torch.float32)


def poison_allocator(ps):
    """Fills the memory the first step's `torch.empty_like` buffers are likely to get with a large value (the test below relies
    only on the zero it asserts, not on this)."""
    junk = [torch.full((p.numel(),), 1e30, device="cuda") for p in ps]
    torch.cuda.synchronize()
    del junk


@pytest.mark.parametrize("stash", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_table_matches_float64_and_agrees_with_the_global_norm(kind, stash):
    g, pa = make_params(31)
    opt = fused(kind, three_groups(pa), track_tensor_stats=True)
    assert opt.track_tensor_stats and opt._controlled() and not opt.track_grad_norm
    zeros = opt.tensor_stats
    assert zeros.dtype == torch.float64 and tuple(zeros.shape) == (len(pa), COLS) and not zeros.any()      # before the first step
    for it in range(2):                                    # step 0 without the late parameter; step 1: its first step beside later ones
        g1, g2 = draw(g, it), draw(g, it)
        applied = hand_over(opt, pa, g1, g2, stash)
        ref = reference(pa, applied, states_of(opt, pa, kind))
        measured = opt.measure_tensor_stats()
        if it == 0:
            poison_allocator(pa)
        opt.step()
        table = opt.tensor_stats
        assert_matches(table, ref, pa, "{} stash={} step {}".format(kind, stash, it))
        assert torch.equal(measured, table)                 # the same pass over the 48-byte rows of measure_tensor_stats()
        if it == 0:
            assert not table[LATE].any()                    # nothing pending: eight zeros
            if not kind.startswith("adam"):
                assert not table[:, 7].any()                # a first SGD step: the fresh momentum buffers are not read
        else:
            assert float(table[0, 7]) > 0.0 and float(table[LATE, 7]) == 0.0
        assert float(table[ZERO, 4]) == pa[ZERO].numel() and float(table[ZERO, 0]) == 0.0
        assert within_one_ulp(norm_of(table), opt.grad_norm), (float(norm_of(table)), float(opt.grad_norm))
    assert int(opt.skipped_steps) == 0


NAN, INF = float("nan"), float("inf")


def plants(n):
    """name -> ([(flat index, value in the stash or None, value in the gradient or None)], count, 1-based first index) for a
    tensor of n elements."""
    mid = min(12345, n - 1)
    cases = {"nan at 0": ([(0, None, NAN)], 1, 1), "nan at the end": ([(n - 1, None, NAN)], 1, n),
             "nan in the stash only": ([(mid, NAN, None)], 1, mid + 1), "nan in the gradient only": ([(mid, None, NAN)], 1, mid + 1),
             "+inf and -inf": ([(mid, INF, -INF)], 1, mid + 1), "3e38 + 3e38": ([(mid, 3e38, 3e38)], 1, mid + 1)}
    if n > 4096:
        cases["nan at 4095"] = ([(4095, None, NAN)], 1, 4096)        # the last element of chunk 0
        cases["nan at 4096"] = ([(4096, None, NAN)], 1, 4097)        # the first of chunk 1
        cases["nan at 4095 and 4096"] = ([(4095, None, NAN), (4096, None, NAN)], 2, 4096)
    return cases


CLEAN = {}


def planted_run(kind, which=None, plant=()):
    """One stashed step of a fresh optimiser over the same parameters and gradients every time, `plant` written into tensor `which`."""
    g, pa = make_params(32)
    opt = fused(kind, three_groups(pa), track_tensor_stats=True)
    g1, g2 = draw(g, 0, late=False), draw(g, 0, late=False)
    for at, v1, v2 in plant:
        if v1 is not None:
            g1[which].view(-1)[at] = v1
        if v2 is not None:
            g2[which].view(-1)[at] = v2
    applied = hand_over(opt, pa, g1, g2, True)
    ref = reference(pa, applied, states_of(opt, pa, kind))
    opt.step()
    return pa, opt.tensor_stats.clone(), ref


# every case in the 85.5-chunk tensor, and in the 1-element tensor where it fits (4095 / 4096 do not exist there)
@pytest.mark.parametrize("which,name", [(w, name) for w in (BIG, ONE) for name in sorted(plants(int(np.prod(SHAPES[w]))))])
@pytest.mark.parametrize("kind", KINDS)
def test_planted_nonfinite_values_are_counted_and_located(kind, which, name):
    plant, count, first = plants(int(np.prod(SHAPES[which])))[name]
    if kind not in CLEAN:
        CLEAN[kind] = planted_run(kind)[1]
        assert not CLEAN[kind][:, 2:4].any()
    pa, table, ref = planted_run(kind, which, plant)
    assert float(table[which, 2]) == count and float(table[which, 3]) == first
    assert_matches(table, ref, pa, "{} {} in tensor {}".format(kind, name, which))
    others = [i for i in range(len(pa)) if i != which]
    assert torch.equal(table[others], CLEAN[kind][others])
    assert float(table[which, 4]) == float(CLEAN[kind][which, 4])      # the planted elements were not zeros


@pytest.mark.parametrize("stash", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_the_table_does_not_depend_on_where_a_gradient_lies(kind, stash):
    tables = []
    for place in (False, True, True):
        g, pa = make_params(33)
        opt = fused(kind, three_groups(pa), track_tensor_stats=True)
        for it in range(2):
            hand_over(opt, pa, draw(g, it), draw(g, it), stash, place=place)
            if place:
                assert pa[BIG].grad.data_ptr() % 16 == 4
            opt.step()
        tables.append(opt.tensor_stats.clone())
    assert float(tables[0][BIG, 0]) > 0.0
    assert torch.equal(tables[0], tables[1]) and torch.equal(tables[1], tables[2])


@pytest.mark.parametrize("kind", KINDS)
def test_a_skipped_step_leaves_its_table_behind(kind):
    g, pa = make_params(34)
    opt = fused(kind, three_groups(pa), skip_nonfinite=True, track_tensor_stats=True)
    captured, at = opt.last_skipped_stats
    hand_over(opt, pa, draw(g, 0, late=False), draw(g, 0, late=False), True)
    opt.step()                                              # step 0: clean
    assert at.dtype == torch.int64 and at.dim() == 0 and int(at) == 0 and not captured.any() and int(opt.skipped_steps) == 0
    snap = all_state(opt, pa, STATE[kind])
    g1, g2 = draw(g, 1), draw(g, 1)
    g2[BIG].view(-1)[4096] = NAN
    hand_over(opt, pa, g1, g2, True)
    opt.step()                                              # step 1: skipped
    captured, at = opt.last_skipped_stats
    bad = opt.tensor_stats.clone()
    assert float(bad[BIG, 2]) == 1 and float(bad[BIG, 3]) == 4097
    assert torch.equal(captured, bad) and int(at) == int(opt.skipped_steps) == 1
    assert all(torch.equal(x, y) for x, y in zip(all_state(opt, pa, STATE[kind]), snap))
    applied = hand_over(opt, pa, draw(g, 2), draw(g, 2), True)
    ref = reference(pa, applied, states_of(opt, pa, kind))
    opt.step()                                              # step 2: clean again
    captured, at = opt.last_skipped_stats
    assert torch.equal(captured, bad) and int(at) == 1 and int(opt.skipped_steps) == 1
    assert not opt.tensor_stats[:, 2].any()
    assert_matches(opt.tensor_stats, ref, pa, kind + " after the skipped step")


@pytest.mark.parametrize("kind", KINDS)
def test_without_skipping_nothing_is_captured(kind):
    g, pa = make_params(35)
    opt = fused(kind, three_groups(pa), track_tensor_stats=True)
    g1 = draw(g, 0)
    g1[ONE].view(-1)[0] = INF
    hand_over(opt, pa, g1, None, False)
    opt.step()
    captured, at = opt.last_skipped_stats
    assert float(opt.tensor_stats[ONE, 2]) == 1 and not captured.any() and int(at) == 0 and int(opt.skipped_steps) == 0


@pytest.mark.parametrize("kind", KINDS)
def test_tracking_is_read_only(kind):
    ga, pa = make_params(36)
    gb, pb = make_params(36)
    oa, ob = fused(kind, three_groups(pa), track_tensor_stats=True), fused(kind, three_groups(pb), track_grad_norm=True)
    for it in range(3):
        hand_over(oa, pa, draw(ga, it), draw(ga, it), True, place=True)
        hand_over(ob, pb, draw(gb, it), draw(gb, it), True, place=True)
        oa.step()
        ob.step()
        assert torch.equal(oa.grad_norm, ob.grad_norm)
    assert all(torch.equal(x, y) for x, y in zip(all_state(oa, pa, STATE[kind]), all_state(ob, pb, STATE[kind])))
    slot = 0 if kind.startswith("adam") else "ctl"
    assert oa._tables[slot][5] is not None and ob._tables[slot][5] is None      # row_of travels only with the option


@pytest.mark.parametrize("kind", KINDS)
def test_off_means_off(kind, monkeypatch):
    from dasac_hip import lib as L

    def refuse(*args):
        raise AssertionError("dasac_tensor_stats called with track_tensor_stats off")
    monkeypatch.setattr(L.load(), "dasac_tensor_stats", refuse)
    for kw in ({}, dict(max_grad_norm=1.0, skip_nonfinite=True, track_grad_norm=True)):
        g, pa = make_params(37)
        opt = fused(kind, three_groups(pa), **kw)
        assert opt.track_tensor_stats is False
        for it in range(2):
            hand_over(opt, pa, draw(g, it), draw(g, it), True)
            opt.step()
        assert opt._stats is None
    opt = fused(kind, three_groups(pa), track_tensor_stats=True)
    hand_over(opt, pa, draw(g, 1), draw(g, 1), True)
    with pytest.raises(AssertionError):                      # control: with the option on the patched entry point is reached
        opt.step()


@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_measuring_changes_nothing(kind, track):
    g, pa = make_params(38)
    opt = fused(kind, three_groups(pa), track_grad_norm=True, track_tensor_stats=track)
    hand_over(opt, pa, draw(g, 0, late=False), draw(g, 0, late=False), True)
    opt.step()
    applied = hand_over(opt, pa, draw(g, 1), draw(g, 1), True)
    grads = [(p.grad, None if p.grad is None else p.grad.clone()) for p in pa]
    stash = {p: (t, t.clone()) for p, t in opt._stash.items()}
    norm, table, before = opt.grad_norm.clone(), opt.tensor_stats.clone(), all_state(opt, pa, STATE[kind])
    first, second = opt.measure_tensor_stats(), opt.measure_tensor_stats()
    assert torch.equal(first, second) and first.data_ptr() != second.data_ptr() != opt.tensor_stats.data_ptr()
    assert_matches(first, reference(pa, applied, states_of(opt, pa, kind)), pa, kind + " measured")
    assert all(p.grad is t and (t is None or torch.equal(t, c)) for p, (t, c) in zip(pa, grads))
    assert set(opt._stash) == set(stash) and all(opt._stash[p] is t and torch.equal(t, c) for p, (t, c) in stash.items())
    assert torch.equal(opt.grad_norm, norm) and torch.equal(opt.tensor_stats, table)
    assert track == bool(table.any())
    assert all(torch.equal(x, y) for x, y in zip(all_state(opt, pa, STATE[kind]), before))
    opt.zero_grad()
    assert not opt.measure_tensor_stats().any()              # nothing pending


def test_bad_arguments_are_refused_and_leave_the_tables_alone():
    from dasac_hip import DasacError
    from dasac_hip import lib as L
    lib = L.load()
    dev = torch.device("cuda")
    p, gr = torch.arange(1.0, 6.0, device=dev), torch.tensor([3.0, 0.0, -4.0, NAN, 0.0], device=dev)
    rows = torch.tensor([[p.data_ptr(), gr.data_ptr(), 0, 0, 5, 0]], dtype=torch.int64, device=dev)
    chunks = torch.zeros(1, 2, dtype=torch.int32, device=dev)
    row_of = torch.tensor([0, -1], dtype=torch.int32, device=dev)
    ws = torch.zeros(lib.dasac_tensor_stats_workspace(1) + 8, dtype=torch.uint8, device=dev)
    assert lib.dasac_tensor_stats_workspace(1) == 64 and lib.dasac_tensor_stats_workspace(0) == 0
    table, captured = torch.full((3, COLS), 7.0, dtype=torch.float64, device=dev), torch.full((3, COLS), 7.0, dtype=torch.float64, device=dev)
    ctl = torch.zeros(4, dtype=torch.float32, device=dev)
    ctl[2:3].view(torch.int32).fill_(1)                      # skip is set
    at, skipped = torch.full((), 7, dtype=torch.int64, device=dev), torch.full((), 5, dtype=torch.int64, device=dev)
    good = dict(tensors=rows.data_ptr(), row_bytes=48, n_tensors=1, chunks=chunks.data_ptr(), n_chunks=1, row_of=row_of.data_ptr(), n_rows=2,
                workspace=ws.data_ptr(), workspace_bytes=64, table=table.data_ptr(), ctl=ctl.data_ptr(), captured=captured.data_ptr(),
                captured_at=at.data_ptr(), skipped=skipped.data_ptr())
    order = list(good)

    def call(**change):
        a = dict(good, **change)
        L.check(lib.dasac_tensor_stats(*[a[k] for k in order], L.stream_ptr()), "dasac_tensor_stats")
    none = dict(ctl=0, captured=0, captured_at=0, skipped=0)
    bad = [dict(row_bytes=40), dict(row_bytes=0), dict(tensors=0), dict(chunks=0), dict(row_of=0), dict(workspace=0), dict(table=0),
           dict(table=table.data_ptr() + 4), dict(workspace=ws.data_ptr() + 4), dict(captured=captured.data_ptr() + 4),
           dict(captured_at=at.data_ptr() + 4), dict(skipped=skipped.data_ptr() + 4), dict(ctl=ctl.data_ptr() + 8),
           dict(n_tensors=0), dict(n_chunks=0), dict(n_rows=0), dict(n_tensors=-1), dict(n_chunks=-1), dict(n_rows=-2), dict(workspace_bytes=63)]
    bad += [{k: 0} for k in none]                            # three of the four given
    bad += [dict(none, **{k: good[k]}) for k in none]        # one of the four given
    for change in bad:
        with pytest.raises(DasacError):
            call(**change)
    torch.cuda.synchronize()
    assert bool((table == 7.0).all()) and bool((captured == 7.0).all()) and int(at) == 7 and int(skipped) == 5
    expect = torch.tensor([[25.0, 4.0, 1.0, 4.0, 2.0, 55.0, 5.0, 0.0], [0.0] * COLS], dtype=torch.float64)
    call(**none)                                             # measure only
    assert torch.equal(table[:2].cpu(), expect) and bool((table[2] == 7.0).all()) and bool((captured == 7.0).all()) and int(at) == 7
    table.fill_(7.0)
    call()                                                   # skip is set: captured too
    assert torch.equal(table[:2].cpu(), expect) and torch.equal(captured[:2].cpu(), expect) and bool((captured[2] == 7.0).all())
    assert int(at) == 5 and int(skipped) == 5
    call(workspace=ws.data_ptr() + 8)                        # 8-byte alignment is enough
    assert torch.equal(table[:2].cpu(), expect)


def test_one_real_model_iteration_reports_every_tensor_without_aten_arithmetic(sac_net):
    import driver
    from test_gpu_no_aten_compute import Recorder
    cfg, net, src, tgt = sac_net
    net.backbone.load_state_dict(rn101_state(3), strict=True)
    optim = driver.make_optimizer(net, cfg, tensor_stats=True, skip_nonfinite=True)
    assert optim.track_tensor_stats and optim.skip_nonfinite
    clone = lambda: (tgt[0], tgt[1].clone(), tgt[2], tgt[3], tgt[4])
    driver.sac_train_iteration(net, optim, src, clone(), 2, True, cfg.LR_TARGET)          # first call: teacher init, caches
    with Recorder() as rec:
        driver.sac_train_iteration(net, optim, src, clone(), 2, True, cfg.LR_TARGET)
        torch.cuda.synchronize()
    assert not rec.big, sorted(set(rec.big))[:12]
    report = driver.gradient_report(net, optim)
    names = [t["name"] for t in report["tensors"]]
    assert len(names) == len(set(names)) == 320 and set(names) <= {n for n, _ in net.named_parameters()}
    assert abs(sum(t["share"] for t in report["tensors"]) - 1.0) <= 1e-12
    assert abs(sum(gr["share"] for gr in report["groups"]) - 1.0) <= 1e-12
    assert report["grad_norm"] > 0.0 and report["nonfinite"] == [] and int(optim.skipped_steps) == 0
    assert within_one_ulp(torch.tensor(report["grad_norm"], dtype=torch.float64).to(torch.float32), optim.grad_norm.cpu())
    assert all(t["first_nonfinite"] is None and t["nonfinite"] == 0 for t in report["tensors"])
    live = [t for t in report["tensors"] if t["grad_norm"] > 0.0]
    assert live and all(t["weight_norm"] > 0.0 and t["state_norm"] > 0.0 and t["update_ratio"] > 0.0 for t in live)
    text = driver.format_gradient_report(report, top=5)
    assert report["top"][0] in text and len(text.split("\n")) == 1 + 5 + len(report["groups"]) + 1
    skipped = driver.skipped_step_report(net, optim)
    assert skipped["captured_at"] == 0 and skipped["grad_norm"] == 0.0
