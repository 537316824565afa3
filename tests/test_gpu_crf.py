"""`dasac_crf_meanfield` on the GPU: against tests/crf_ref.py in float64 with the project's yardstick
    err(HIP vs fp64) <= 2 * err(crf_ref in float32 on the CPU vs fp64) + 1e-6
for probs_out and conf, labels exact outside the exempt pixels (float64 top-two gap <= twice the allowed absolute Q error;
test_crf_cpu.py caps them at 0.5 % per case and finds none); the identities of the definition on the device; guarded operands at every
alignment phase on exactly the workspace asked for; refused arguments; and driver.infer_label_maps_ms / validation_iou with `crf`.
Every ratio is printed before it is asserted (profiles/crf_meanfield.md keeps a copy)."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import boundary_ref as BR
import crf_ref as CR
from crf import CrfParams
from exact_workspace import ExactWorkspace
from fp64_yardstick import _ratio, _report
from guarded_operands import Arena, bits_equal
from test_gpu_infer_fused import net  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

EINVAL, EWORKSPACE = -1, -2
SENTINEL = 0x5C
IDS = lambda c: "x".join(map(str, c))


def _run(P, I, params, **kw):
    from dasac_hip import ops
    return ops.crf_meanfield(P.cuda(), I.cuda(), params, **kw)


# ---- float64 parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CR.CASES, ids=IDS)
def test_crf_meanfield_matches_float64(case):
    P, I, params, Q64, Q32 = CR.case_reference(case)
    B, C, H, W = P.shape
    labels, conf, probs = _run(P, I, params, want_conf=True, want_probs=True)
    assert labels.dtype == torch.uint8 and tuple(labels.shape) == (B, H, W)
    assert conf.dtype == torch.float32 and tuple(conf.shape) == (B, H, W) and tuple(probs.shape) == (B, C, H, W)
    lab64, conf64, _ = CR.labels_of(Q64)
    exempt = CR.exempt_pixels(case)
    differ = labels.cpu().long() != lab64
    print("crf_meanfield {}: {} labels differ from float64, {} pixels exempt".format(case, int(differ.sum()), int(exempt.sum())))
    _report("crf_meanfield", case, {"probs": _ratio(probs, Q64, Q32), "conf": _ratio(conf, conf64, Q32.max(1).values)})
    assert not bool((differ & ~exempt).any())
    assert torch.equal(conf, probs.max(1).values) and torch.equal(labels.long(), probs.argmax(1))
    # labels alone, and through a LUT: the same map
    alone = _run(P, I, params)
    assert alone[1] is None and alone[2] is None and torch.equal(alone[0], labels)
    lut = torch.arange(255, 255 - 32, -1, dtype=torch.uint8).cuda()
    through, conf_l, none = _run(P, I, params, lut=lut, want_conf=True)
    assert none is None and torch.equal(conf_l, conf) and torch.equal(through, lut[labels.long()])


# ---- identities -------------------------------------------------------------------------------------------------------------------
def test_no_compatibility_returns_p_renormalised_on_the_device():
    P, I, _ = CR.scene(2, 19, 21, 70, 5)
    P = (P * torch.rand(2, 1, 21, 70, generator=torch.Generator().manual_seed(6)).clamp_min(0.1)).contiguous()
    _, _, probs = _run(P, I, CrfParams(compat=0.0, n_iter=3), want_probs=True)
    want = P.double() / P.double().sum(1, keepdim=True)
    _report("crf_meanfield compat = 0", tuple(P.shape), {"probs": _ratio(probs, want, P / P.sum(1, keepdim=True))})


def test_one_hot_probabilities_keep_their_labels_on_the_device():
    _, I, gt = CR.scene(2, 19, 21, 70, 7)
    lab = torch.randint(0, 19, gt.shape, generator=torch.Generator().manual_seed(8))
    P = torch.nn.functional.one_hot(lab, 19).permute(0, 3, 1, 2).float().contiguous()
    labels, conf, _ = _run(P, I, CrfParams(), want_conf=True)
    assert torch.equal(labels.cpu().long(), lab)
    assert float((conf.cpu() - 1).abs().max()) <= 1e-6


@pytest.mark.parametrize("case", [CR.CASES[1], CR.CASES[2]], ids=IDS)
def test_mirroring_the_inputs_mirrors_the_result_on_the_device(case):
    P, I, params, Q64, Q32 = CR.case_reference(case)
    ratios = {}
    for name, dims in (("x", (-1,)), ("y", (-2,)), ("xy", (-1, -2))):
        _, conf, probs = _run(P.flip(dims).contiguous(), I.flip(dims).contiguous(), params, want_conf=True, want_probs=True)
        ratios["probs " + name] = _ratio(probs, Q64.flip(dims), Q32.flip(dims))
        ratios["conf " + name] = _ratio(conf, Q64.max(1).values.flip(dims), Q32.max(1).values.flip(dims))
    _report("crf_meanfield mirrored", case, ratios)


# ---- placement and contract -------------------------------------------------------------------------------------------------------
def _guarded_run(monkeypatch, case, arena):
    from dasac_hip import lib as L, ops
    P, I, params, _, _ = CR.case_reference(case)
    guard = ExactWorkspace()
    with monkeypatch.context() as m:
        m.setattr(ops, "torch", arena.torch)
        m.setattr(L, "workspace", guard)
        lut = arena.place(torch.arange(40, 40 + 19, dtype=torch.uint8))
        outs = ops.crf_meanfield(arena.place(P), arena.place(I), params, lut=lut, want_conf=True, want_probs=True)
    arena.check()
    assert guard.check() == 1 and guard.requests[0][0] == L.load().dasac_crf_meanfield_workspace(*case[:4], case[6])
    assert all(arena.owns(t) for t in outs)
    return outs


def test_crf_meanfield_on_guarded_operands_at_every_phase_on_the_exact_workspace(monkeypatch):
    """The 37 x 53 case (odd H * W: the planes sit at every 4-byte phase): the guards of the operands and of the workspace stay
    intact, the inputs unchanged, and the three outputs bit-equal across the base phases 0, 4, 8, 12 bytes and across two runs."""
    case = CR.CASES[1]
    plain, again = _guarded_run(monkeypatch, case, Arena(None)), _guarded_run(monkeypatch, case, Arena(None))
    for i, (a, b) in enumerate(zip(plain, again)):
        assert bits_equal(a, b), "output {}: two runs differ".format(i)
    for phase in range(4):
        got = _guarded_run(monkeypatch, case, Arena(phase))
        for i, (a, b) in enumerate(zip(plain, got)):
            assert bits_equal(a, b), "output {} at base phase {} differs from the plain run".format(i, phase)


def _raw(P, I, params, labels, conf, probs, ws_ptr, ws_bytes, lut=None, shape=None, Ci=None):
    """dasac_crf_meanfield itself; `params` anything with the nine fields; returns the code."""
    from dasac_hip import lib as L
    B, C, H, W = shape or P.shape
    return L.load().dasac_crf_meanfield(P.data_ptr(), I.data_ptr(), B, C, I.shape[1] if Ci is None else Ci, H, W, params.radius, params.dilation,
                                        params.w_app, params.theta_alpha, params.theta_beta, params.w_smooth, params.theta_gamma,
                                        params.compat, params.n_iter, L.ptr(lut), L.ptr(labels), L.ptr(conf), L.ptr(probs), ws_ptr, ws_bytes,
                                        L.stream_ptr())


def _filled(shape, dtype=torch.float32):
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(-1).view(torch.uint8).fill_(SENTINEL)
    return t


def _untouched(*tensors):
    torch.cuda.synchronize()
    return all(bool((t.view(-1).view(torch.uint8) == SENTINEL).all()) for t in tensors)


@pytest.mark.parametrize("n_iter", [1, 3])
def test_crf_meanfield_refuses_a_workspace_one_byte_short(n_iter):
    from dasac_hip import lib as L
    lib = L.load()
    B, C, H, W = 2, 19, 37, 53
    P, I, _ = CR.scene(B, C, H, W, 1)
    P, I = P.cuda(), I.cuda()
    params = CrfParams(radius=2, dilation=3, n_iter=n_iter)
    need = lib.dasac_crf_meanfield_workspace(B, C, H, W, n_iter)
    assert need == (1 if n_iter == 1 else 2) * ((B * C * H * W * 4 + 15) // 16 * 16)
    guard = ExactWorkspace()
    ws = guard(need, P.device)
    labels, conf, probs = _filled((B, H, W), torch.uint8), _filled((B, H, W)), _filled((B, C, H, W))
    assert _raw(P, I, params, labels, conf, probs, ws.data_ptr(), need - 1) == EWORKSPACE
    assert b"workspace" in lib.dasac_last_error()
    assert _untouched(labels, conf, probs) and bool((ws == 0xFF).all()) and guard.check() == 1
    assert _raw(P, I, params, labels, conf, probs, ws.data_ptr(), need) == 0, lib.dasac_last_error()
    assert guard.check() == 1
    want = _run(P, I, params, want_conf=True, want_probs=True)
    assert all(bits_equal(a, b) for a, b in zip((labels, conf, probs), want))


# ---- argument errors --------------------------------------------------------------------------------------------------------------
def test_crf_meanfield_refuses_bad_arguments_and_leaves_the_outputs_alone():
    from dasac_hip import lib as L, ops, DasacError
    lib = L.load()
    B, C, H, W = 1, 19, 6, 9
    P, I, _ = CR.scene(B, C, H, W, 2)
    P, I = P.cuda(), I.cuda()
    big_p, big_i = torch.rand(B, 33, H, W).cuda(), torch.randn(B, 5, H, W).cuda()
    good = NS(**CrfParams().as_dict())
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    labels, conf, probs = _filled((B, H, W), torch.uint8), _filled((B, H, W)), _filled((B, 33, H, W))
    change = lambda **kw: NS(**dict(vars(good), **kw))

    def refused(params=good, p=P, i=I, **kw):
        rc = _raw(p, i, params, labels, conf, probs, ws.data_ptr(), ws.numel(), **kw)
        assert b"crf_meanfield" in lib.dasac_last_error()
        return rc == EINVAL and _untouched(labels, conf, probs)
    assert refused(change(radius=6)) and refused(change(radius=0))
    assert refused(change(radius=3, dilation=3)) and refused(change(dilation=5, radius=1)) and refused(change(dilation=0))
    assert refused(p=big_p) and refused(shape=(B, 0, H, W))
    assert refused(i=big_i) and refused(Ci=0)
    assert refused(change(n_iter=0)) and refused(change(n_iter=17))
    assert refused(change(theta_beta=0.0)) and refused(change(theta_alpha=-1.0)) and refused(change(theta_gamma=float("nan")))
    assert refused(change(w_app=0.0, w_smooth=0.0)) and refused(change(w_smooth=-0.5))
    assert refused(change(compat=-1.0)) and refused(change(compat=float("inf")))
    assert refused(shape=(0, C, H, W)) and refused(shape=(B, C, 0, W)) and refused(shape=(B, C, H, -1))
    assert _raw(P, I, good, labels, conf, P, ws.data_ptr(), ws.numel()) == EINVAL               # probs_out is probs
    assert _raw(P, I, good, labels, conf, P[:, 1:], ws.data_ptr(), ws.numel()) == EINVAL        # ... overlaps it
    assert _raw(P, I, good, labels, I, None, ws.data_ptr(), ws.numel()) == EINVAL               # conf is the image
    assert _raw(P, I, good, labels, conf, None, P.data_ptr(), P.numel() * 4, shape=(B, 9, H, W)) == EINVAL     # the workspace lies in probs
    assert _raw(P, I, good, None, conf, None, ws.data_ptr(), ws.numel()) == EINVAL and _raw(P, I, good, labels, conf, None, 0, 0) == EINVAL
    assert _untouched(labels, conf, probs)
    before = P.clone(), I.clone()
    assert _raw(P, I, good, labels, conf, probs, ws.data_ptr(), ws.numel()) == 0, lib.dasac_last_error()
    assert not _untouched(labels) and torch.equal(P, before[0]) and torch.equal(I, before[1])
    # through the wrapper: DasacError
    for bad in (change(radius=6), change(radius=3, dilation=3), change(n_iter=0), change(theta_beta=0.0)):
        with pytest.raises(DasacError):
            ops.crf_meanfield(P, I, bad)
    with pytest.raises(DasacError):
        ops.crf_meanfield(big_p, I, good)                                  # C = 33
    with pytest.raises(DasacError):
        ops.crf_meanfield(P, big_i, good)                                  # Ci = 5
    for image in (I[:, :, :-1], I[:, :, :, :-1], torch.cat([I, I]), I[0], I.double()):     # mismatched shapes and types
        with pytest.raises(DasacError):
            ops.crf_meanfield(P, image, good)
    with pytest.raises(DasacError):
        ops.crf_meanfield(P.cpu(), I.cpu(), good)


# ---- through the model ------------------------------------------------------------------------------------------------------------
PARAMS = CrfParams(radius=3, dilation=2, n_iter=3)


def test_infer_label_maps_ms_with_crf_is_crf_refine_of_its_own_probabilities(net):  # noqa: F811
    import driver
    x = torch.randn(2, 3, 33, 49, generator=torch.Generator().manual_seed(1)).cuda()
    kw = dict(scales=(0.75, 1.0), flip=True, lut=driver.CITYSCAPES_TRAIN_TO_ID, want_conf=True, want_probs=True)
    plain = driver.infer_label_maps_ms(net, x, **kw)
    refined = driver.infer_label_maps_ms(net, x, crf=PARAMS, **kw)
    by_hand = driver.crf_refine(plain[2], x, PARAMS, driver.CITYSCAPES_TRAIN_TO_ID, True, True)
    assert all(bits_equal(a, b) for a, b in zip(refined, by_hand))
    assert refined[0].dtype == torch.uint8 and set(refined[0].unique().tolist()) <= set(driver.CITYSCAPES_TRAIN_TO_ID)
    assert not bits_equal(refined[2], plain[2])
    lab, conf, probs = driver.infer_label_maps_ms(net, x, scales=(1.0,), flip=False, crf=PARAMS)
    assert conf is None and probs is None and lab.dtype == torch.uint8 and int(lab.max()) < 19


def test_infer_label_maps_ms_without_crf_never_enters_the_crf(net, monkeypatch):  # noqa: F811
    import driver
    from dasac_hip import ops
    calls = []
    inner = ops.crf_meanfield
    monkeypatch.setattr(ops, "crf_meanfield", lambda *a, **k: (calls.append(1), inner(*a, **k))[1])
    x = torch.randn(2, 3, 33, 49, generator=torch.Generator().manual_seed(1)).cuda()
    kw = dict(scales=(0.75, 1.0), flip=True, want_conf=True, want_probs=True)
    without = driver.infer_label_maps_ms(net, x, **kw)
    with_none = driver.infer_label_maps_ms(net, x, crf=None, **kw)
    assert all(bits_equal(a, b) for a, b in zip(without, with_none)) and not calls
    driver.infer_label_maps_ms(net, x, crf=PARAMS, **kw)
    assert calls == [1]


def test_validation_iou_with_crf_counts_the_refined_maps(net, monkeypatch):  # noqa: F811
    import driver
    g = torch.Generator().manual_seed(3)
    batches = []
    for _ in range(2):
        gt = torch.randint(0, 19, (1, 33, 49), generator=g)
        gt[torch.rand(1, 33, 49, generator=g) < 0.2] = 255
        batches.append((torch.randn(1, 3, 33, 49, generator=g).cuda(), gt.cuda()))
    seen = []
    summarise = driver.summarise_iou
    monkeypatch.setattr(driver, "summarise_iou", lambda counts: (seen.append(counts.clone()), summarise(counts))[1])
    R = 2
    miou, iou, table = driver.validation_iou(net, batches, crf=PARAMS, boundary_radius=R)
    want, want_table, changed = np.zeros((3, 19), np.int64), np.zeros((R + 1, 5, 19), np.int64), 0
    for image, gt in batches:
        pred = driver.infer_label_maps_ms(net, image, scales=(1.0,), flip=False, crf=PARAMS)[0]
        changed += int((pred != driver.infer_label_maps_ms(net, image, scales=(1.0,), flip=False)[0]).sum())
        want += BR.mask_counts_ref(pred.cpu().numpy(), gt.cpu().numpy(), 19)
        want_table += BR.boundary_table(pred.cpu().numpy(), gt.cpu().numpy(), 19, R)
    print("validation_iou with crf: {} of {} pixels changed their label".format(changed, 2 * 33 * 49))
    assert len(seen) == 1 and np.array_equal(seen[0].cpu().numpy(), want)
    assert table.dtype == torch.int64 and not table.is_cuda and np.array_equal(table.numpy(), want_table)
    assert torch.equal(iou, summarise(torch.from_numpy(want))[0]) and miou == float(iou.mean())
    # the same through an explicit multi-scale call; and without crf nothing changed
    assert driver.validation_iou(net, batches, scales=(1.0,), crf=PARAMS, boundary_radius=R)[0] == miou
    assert not net.training
