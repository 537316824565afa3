"""`dasac_label_segments`, `dasac_segment_counts` and `dasac_segment_filter` on the GPU against the numpy model of
tests/segments_ref.py, bit for bit: integer maps and tables, so every comparison is exact.  Shapes of one pixel, one row, one
column, one tile less / exactly / one more than a tile each way, several tiles, an odd width; uniform, empty, checkerboard,
diagonal, serpentine, spiral, ring, comb, row-wrap and seeded random maps under both connectivities; int64 maps with -1 and 200 and
uint8 maps off their alignment; the layer slots, ties in the arg-max, accumulation and the sums over the bins against
`ops.mask_counts`; refused arguments; exact workspaces and guarded operands at every phase; and `driver.validation` /
`driver.despeckle` end to end."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.utils._python_dispatch import TorchDispatchMode

import boundary_ref as BR
import segments_ref as SR
from dasac_hip.ops import SEGMENT_TILE
from exact_workspace import ExactWorkspace
from guarded_operands import Arena, bits_equal

pytestmark = pytest.mark.gpu

EINVAL = -1
TH, TW = SEGMENT_TILE
C19 = 19
# one pixel, one row, one column; a tile less one, a tile, a tile and one; several tiles (seams both ways, corners); an odd width
SHAPES = [(1, 1), (1, 7), (7, 1), (TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1), (2 * TH + 3, 2 * TW + 5), (TH + 5, TW + 7)]
SHAPE_IDS = ["{}x{}".format(*s) for s in SHAPES]
COUNT_SHAPES = [(1, 1), (7, 1), (TH, TW), (TH + 1, TW + 1), (2 * TH + 3, 2 * TW + 5)]
NAMED = ["uniform", "empty", "checkerboard", "diagonals", "serpentine", "spiral", "rings", "comb", "u_shape", "row_wrap", "row_wrap_next"]


def _patterns(H, W):
    """[(name, int64 [H,W])]: the named patterns, then seeded random maps of 2, 3 and 19 classes at scales 1, 3 and 8."""
    rng = np.random.default_rng(1000 * H + W)
    maps = [SR.uniform(H, W, 1), np.full((H, W), 255, np.int64), SR.checkerboard(H, W), SR.diagonals(H, W), SR.serpentine(H, W),
            SR.spiral(H, W), SR.rings(H, W), SR.comb(H, W), SR.comb(H, W, pitch=max(1, W - 1)), SR.row_wrap(H, W), SR.row_wrap(H, W)]
    out = list(zip(NAMED, maps))
    out += [("random{}_{}".format(C, scale), SR.random_map(H, W, C, scale, rng)) for C in (2, 3, 19) for scale in (1, 3, 8)]
    return out


def _batches(n):
    """Index ranges over n images: a batch of 1, then batches of 3 (different content per image), the last as long as it gets."""
    cuts = [0, 1] + list(range(4, n, 3)) + [n]
    return [(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]


def _place(t, offset):
    """`t` on the device, starting `offset` ELEMENTS into its allocation."""
    flat = torch.empty(t.numel() + offset, dtype=t.dtype, device="cuda")
    view = flat[offset:].view(t.shape)
    view.copy_(t)
    return view


@pytest.fixture(scope="module")
def models():
    """Per shape: the pattern names, the maps [N,H,W] and the model's (roots, sizes) per connectivity -- computed once."""
    out = {}
    for H, W in SHAPES:
        names, maps = zip(*_patterns(H, W))
        maps = np.stack(maps)
        out[(H, W)] = (list(names), maps, {conn: SR.segments(maps, C19, conn) for conn in (4, 8)})
    return out


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("H,W", SHAPES, ids=SHAPE_IDS)
def test_label_segments_match_the_model_bit_for_bit(models, H, W, connectivity):
    from dasac_hip import ops
    names, maps, want = models[(H, W)]
    roots, sizes = want[connectivity]
    as_i64 = maps.copy()
    as_i64[(maps == 255) & (np.arange(W)[None, None, :] % 2 == 0)] = -1           # int64 maps: -1 and 200 are no class as 255 is
    as_i64[(maps == 255) & (np.arange(W)[None, None, :] % 2 == 1)] = 200
    for a, b in _batches(len(maps)):
        d_i64 = _place(torch.from_numpy(as_i64[a:b]), 1)
        d_u8 = _place(torch.from_numpy(maps[a:b].astype(np.uint8)), 1 + a % 4)    # odd byte offsets among them
        assert d_i64.data_ptr() % 16 == 8 and (a % 2 == 1 or d_u8.data_ptr() % 2 == 1)
        seg, size = ops.label_segments(d_i64, C19, connectivity)
        assert seg.dtype == torch.int32 and size.dtype == torch.int32 and tuple(seg.shape) == (b - a, H, W)
        assert np.array_equal(seg.cpu().numpy(), roots[a:b]), names[a:b]
        assert np.array_equal(size.cpu().numpy(), sizes[a:b]), names[a:b]
        seg8, size8 = ops.label_segments(d_u8, C19, connectivity)
        assert torch.equal(seg8, seg) and torch.equal(size8, size), names[a:b]
        again, none = ops.label_segments(d_i64, C19, connectivity, want_size=False)     # a second run: the same bits
        assert none is None and torch.equal(again, seg)
    # what the patterns promise, on the device's own output
    seg, size = ops.label_segments(torch.from_numpy(maps[:4]).cuda(), C19, connectivity)
    assert int(seg[0].max()) == 0 and int(size[0].min()) == H * W                              # uniform: one segment, root 0
    assert int(seg[1].max()) == -1 and int(size[1].max()) == 0                                 # all 255
    n_checker = len(torch.unique(seg[2]))
    assert n_checker == (H * W if connectivity == 4 or min(H, W) == 1 else 2)
    if connectivity == 8 and min(H, W) >= 3:
        assert int(size[3][torch.from_numpy(maps[3] == 2).cuda()].max()) > 1                   # diagonals hold together under 8 only
    if connectivity == 4:
        assert int(size[3][torch.from_numpy(maps[3] == 2).cuda()].max()) == 1
    if H >= 6 and W >= 3:                                                                      # the row-wrap runs stay apart
        k = NAMED.index("row_wrap")
        pair, pair_size = ops.label_segments(torch.from_numpy(maps[k:k + 2]).cuda(), 2, connectivity)
        assert int(pair_size[0, 2, W - 1]) == 1 and int(pair_size[0, 3, 0]) == 1
        assert int(pair_size[0, H - 1, 0]) == W and int(pair_size[1, 0, 0]) == W and int(pair[1, 0, W - 1]) == 0


def test_label_segments_with_255_classes():
    from dasac_hip import ops
    rng = np.random.default_rng(5)
    H, W = TH + 3, TW + 9
    m = BR.blocky((2, H, W), list(range(256)), 2, rng).astype(np.int64)
    m[1] = np.arange(H * W).reshape(H, W) % 255                                  # every class 0..254 in a row, 254 next to 0
    roots, sizes = SR.segments(m, 255, 8)
    assert (roots[0] == -1).any() and (m[0] == 254).any()                        # 255 is no class, 254 is one
    for d in (torch.from_numpy(m).cuda(), torch.from_numpy(m.astype(np.uint8)).cuda()):
        seg, size = ops.label_segments(d, 255, 8)
        assert np.array_equal(seg.cpu().numpy(), roots) and np.array_equal(size.cpu().numpy(), sizes)


# ---------------------------------------------------------------------------------------------------------------------
# segment_counts
# ---------------------------------------------------------------------------------------------------------------------
def _count_case(H, W, C=C19):
    """Three images of different content: a blocky ground truth with 255 and -1, a serpentine through classes, random blocks.  A
    label map that is the ground truth with specks and 255 holes, four score tensors (one-hot of noisy maps; random with exact
    ties; all zero: class 0 by ties) and the ground truth itself."""
    rng = np.random.default_rng(77 * H + W)
    gt = np.stack([BR.blocky((1, H, W), list(range(C)) + [255, -1], 5, rng)[0], SR.serpentine(H, W, 3, 4), SR.random_map(H, W, 5, 8, rng)])
    gt = gt.astype(np.int64)
    gt[0, H // 2, W // 2] = 255

    def noisy(share):
        m = gt.copy()
        specks = rng.random(m.shape) < share
        m[specks] = rng.integers(0, C, int(specks.sum()))
        return m
    labels = noisy(0.05)
    labels[rng.random(labels.shape) < 0.05] = 255
    one_hot = lambda m: (np.arange(C)[None, :, None, None] == np.where((m >= 0) & (m < C), m, 1)[:, None]).astype(np.float32)
    s0, s2 = one_hot(noisy(0.2)), one_hot(noisy(0.02))
    s1 = rng.standard_normal((3, C, H, W)).astype(np.float32)
    a, b = W // 3, 2 * W // 3
    s1[0, :, :, :a] = s1[0, :1, :, :a]                                           # exact ties over all classes: class 0
    if C > 2:
        s1[0, 2, :, a:b] = s1[0, 1, :, a:b] = np.abs(s1[0, :, :, a:b]).max(0) + 1.0     # a two-way tie at the top: class 1
    s3 = np.zeros((3, C, H, W), np.float32)                                      # uniform by ties: class 0
    return [s0, s1, s2, s3], labels, gt


@pytest.fixture(scope="module")
def count_cases():
    out = {}
    for H, W in COUNT_SHAPES:
        scores, labels, gt = _count_case(H, W)
        out[(H, W)] = (scores, labels, gt, {conn: SR.segment_tables(scores, [labels, labels], gt, C19, conn) for conn in (4, 8)})
    return out


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("H,W", COUNT_SHAPES, ids=["{}x{}".format(*s) for s in COUNT_SHAPES])
def test_segment_counts_match_the_model_bit_for_bit(count_cases, H, W, connectivity):
    from dasac_hip import ops
    scores, labels, gt, want = count_cases[(H, W)]
    want = want[connectivity]
    d_scores = [_place(torch.from_numpy(s), 1) for s in scores]
    d_gt = _place(torch.from_numpy(gt), 1)
    d_i64 = _place(torch.from_numpy(labels), 1)
    d_u8 = _place(torch.from_numpy(labels.astype(np.uint8)), 1)
    assert d_u8.data_ptr() % 2 == 1 and (H * W < 1000 or (gt.min() == -1 and (gt == 255).any() and (labels == 255).any()))
    got = ops.segment_counts(d_scores, [d_i64, d_u8], d_gt, connectivity=connectivity)
    assert got.dtype == torch.int64 and tuple(got.shape) == (6, 2, 24, 4, C19)
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(got[4], got[5])                                          # the same map as int64 and as uint8
    assert int(got[:, 0, :, 0].sum()) > 0 and int(got[:, 1, :, 0].sum()) > 0
    # summed over the bins: ops.mask_counts on the same tensors
    plain = ops.mask_counts(d_scores, [d_i64], d_gt)
    s = got.sum(2)
    for l in range(5):
        tp, fp, fn = plain[l]
        assert torch.equal(s[l, 0, 2], tp) and torch.equal(s[l, 0, 1], tp + fn), l
        assert torch.equal(s[l, 1, 1], tp + fp) and torch.equal(s[l, 1, 2], tp), l
    # two calls accumulate; two runs give the same bits
    again = ops.segment_counts(d_scores, [d_i64, d_u8], d_gt, got.clone(), connectivity)
    assert torch.equal(again, 2 * got)
    # label maps alone; another ignore_index (class 3 is no class in the ground-truth map, still one in the predicted maps)
    alone = ops.segment_counts([], [d_u8], d_gt, connectivity=connectivity, num_classes=C19)
    assert torch.equal(alone[0], got[5])
    other = ops.segment_counts([d_scores[1]], [d_i64], d_gt, connectivity=connectivity, ignore_index=3)
    assert np.array_equal(other.cpu().numpy(), SR.segment_tables([scores[1]], [labels], gt, C19, connectivity, 3))


def test_segment_counts_number_the_layers_over_the_non_null_slots(count_cases):
    from dasac_hip import lib as L, ops
    lib = L.load()
    H, W = COUNT_SHAPES[3]
    scores, labels, gt, want = count_cases[(H, W)]
    s1, m, d_gt = torch.from_numpy(scores[1]).cuda(), torch.from_numpy(labels.astype(np.uint8)).cuda(), torch.from_numpy(gt).cuda()
    table = torch.zeros(2, 2, 24, 4, C19, dtype=torch.int64, device="cuda")
    ws = torch.empty(lib.dasac_segment_counts_workspace(2, 3, H, W), dtype=torch.uint8, device="cuda")
    rc = lib.dasac_segment_counts(0, 0, s1.data_ptr(), 0, 0, m.data_ptr(), 2, d_gt.data_ptr(), 3, C19, H, W, 8, 255, table.data_ptr(),
                                  ws.data_ptr(), ws.numel(), L.stream_ptr())
    assert rc == 0, lib.dasac_last_error()
    assert np.array_equal(table.cpu().numpy(), want[8][[1, 5]])                 # scores2 is layer 0, labels1 (uint8 by bit 1) is layer 1
    assert torch.equal(table, ops.segment_counts([s1], [m], d_gt))


# ---------------------------------------------------------------------------------------------------------------------
# segment_filter
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 7), (TH + 1, TW + 1), (2 * TH + 3, 2 * TW + 5)], ids=["1x7", "tile+1", "tiles"])
def test_segment_filter_matches_the_model_and_leaves_its_input(models, H, W):
    from dasac_hip import ops
    names, maps, model = models[(H, W)]
    keep = [names.index(n) for n in ("uniform", "checkerboard", "rings", "random19_1", "random3_3", "random2_8")]
    maps = maps[keep]
    for dtype in (np.int64, np.uint8):
        host = maps.astype(dtype)
        d = _place(torch.from_numpy(host), 3)
        before = d.clone()
        for connectivity in (4, 8):
            for fill in (255, 0):
                for min_size in (0, 1, 2, 5, H * W, H * W + 1):
                    got = ops.segment_filter(d, min_size, C19, fill, connectivity)
                    assert got.dtype == d.dtype and got.shape == d.shape and got.data_ptr() != d.data_ptr()
                    roots, sizes = (a[keep] for a in model[connectivity])                  # the model's segments, computed once
                    want = np.where((roots >= 0) & (sizes < min_size), np.asarray(fill).astype(dtype), host)
                    assert np.array_equal(got.cpu().numpy(), want), (dtype, connectivity, fill, min_size)
                    if min_size <= 1:
                        assert torch.equal(got, d)
        assert torch.equal(d, before)
    whole = ops.segment_filter(torch.from_numpy(maps[:1]).cuda(), H * W + 1, C19, 7)      # the uniform map goes, as one segment
    assert int((whole != 7).sum()) == 0


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_segment_ops_refuse_bad_arguments_without_a_launch():
    from dasac_hip import lib as L, ops, DasacError
    lib = L.load()
    m = torch.ones(1, 4, 4, dtype=torch.int64, device="cuda")
    m8 = torch.ones(1, 4, 4, dtype=torch.uint8, device="cuda")
    seg = torch.full((1, 4, 4), 77, dtype=torch.int32, device="cuda")
    out = torch.full((1, 4, 4), 77, dtype=torch.int64, device="cuda")
    s = torch.zeros(1, 19, 4, 4, device="cuda")
    big = torch.zeros(1, 65, 4, 4, device="cuda")
    table = torch.zeros(2, 2, 24, 4, 65, dtype=torch.int64, device="cuda")
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    sp = L.stream_ptr()

    def label(labels=m.data_ptr(), u8=0, B=1, C=19, H=4, W=4, conn=8, segment=seg.data_ptr(), size=0):
        return lib.dasac_label_segments(labels, u8, B, C, H, W, conn, segment, size, 0, 0, sp)
    assert label(conn=6) == EINVAL and label(conn=0) == EINVAL and label(C=0) == EINVAL and label(C=256) == EINVAL
    assert b"label_segments" in lib.dasac_last_error()
    assert label(labels=0) == EINVAL and label(segment=0) == EINVAL and label(B=0) == EINVAL and label(H=0) == EINVAL and label(W=-1) == EINVAL
    assert label(H=1 << 16, W=1 << 15) == EINVAL                                 # H * W = 2^31
    assert label(labels=m.data_ptr() + 4) == EINVAL and label(segment=seg.data_ptr() + 2) == EINVAL
    torch.cuda.synchronize()
    assert int((seg != 77).sum()) == 0                                           # nothing was launched
    assert label(C=255) == 0 and label(labels=m8.data_ptr(), u8=1) == 0 and label(conn=4) == 0

    def filt(labels=m.data_ptr(), u8=0, C=19, conn=8, min_size=2, fill=255, o=out.data_ptr(), w=ws.data_ptr(), n=ws.numel()):
        return lib.dasac_segment_filter(labels, u8, 1, C, 4, 4, conn, min_size, fill, o, w, n, sp)
    need = lib.dasac_segment_filter_workspace(1, 4, 4)
    assert need > 0 and lib.dasac_label_segments_workspace(1, 4, 4) == 0
    assert filt(conn=6) == EINVAL and filt(C=0) == EINVAL and filt(C=256) == EINVAL
    assert filt(o=m.data_ptr()) == EINVAL and filt(o=m.data_ptr() + 8) == EINVAL      # out aliases / overlaps labels
    assert b"segment_filter" in lib.dasac_last_error() and b"alias" in lib.dasac_last_error()
    assert filt(n=need - 1) == EINVAL and filt(w=0) == EINVAL and filt(w=ws.data_ptr() + 4) == EINVAL
    assert filt(labels=m8.data_ptr(), u8=1, fill=256) == EINVAL
    torch.cuda.synchronize()
    assert int((out != 77).sum()) == 0
    assert filt(n=need) == 0 and filt(min_size=0) == 0

    def counts(s0=s.data_ptr(), m0=m.data_ptr(), gt=m.data_ptr(), B=1, C=19, conn=8, t=table.data_ptr(), w=ws.data_ptr(), n=ws.numel()):
        return lib.dasac_segment_counts(s0, 0, 0, 0, m0, 0, 0, gt, B, C, 4, 4, conn, 255, t, w, n, sp)
    assert counts(conn=6) == EINVAL and counts(C=0) == EINVAL and counts(s0=big.data_ptr(), C=65) == EINVAL
    assert b"segment_counts" in lib.dasac_last_error()
    assert counts(s0=0, m0=0) == EINVAL and counts(gt=0) == EINVAL and counts(t=0) == EINVAL and counts(w=0) == EINVAL and counts(B=0) == EINVAL
    assert counts(n=lib.dasac_segment_counts_workspace(2, 1, 4, 4) - 1) == EINVAL
    assert counts(w=ws.data_ptr() + 4) == EINVAL and counts(gt=m.data_ptr() + 4) == EINVAL
    torch.cuda.synchronize()
    assert int(table.sum()) == 0
    assert counts(n=lib.dasac_segment_counts_workspace(2, 1, 4, 4)) == 0 and counts(s0=big.data_ptr(), C=64) == 0
    # the wrappers: wrong dtypes, CPU tensors, classes, connectivity -- DasacError naming the op
    for call in (lambda: ops.label_segments(m.to(torch.int32), 19), lambda: ops.label_segments(m.cpu(), 19),
                 lambda: ops.label_segments(m, 19, connectivity=6), lambda: ops.label_segments(m, 0), lambda: ops.label_segments(m, 256),
                 lambda: ops.label_segments(m[0], 19)):
        with pytest.raises(DasacError, match="label_segments"):
            call()
    for call in (lambda: ops.segment_filter(m.to(torch.float32), 2, 19), lambda: ops.segment_filter(m8.cpu(), 2, 19),
                 lambda: ops.segment_filter(m, 2, 19, connectivity=6), lambda: ops.segment_filter(m, 2, 256),
                 lambda: ops.segment_filter(m8, 2, 19, fill=-1)):
        with pytest.raises(DasacError, match="segment_filter"):
            call()
    for call in (lambda: ops.segment_counts([], [], m), lambda: ops.segment_counts([s.cpu()], [], m.cpu()),
                 lambda: ops.segment_counts([s], [], m, connectivity=6), lambda: ops.segment_counts([big], [], m),
                 lambda: ops.segment_counts([], [m], m), lambda: ops.segment_counts([s], [m.to(torch.int32)], m),
                 lambda: ops.segment_counts([s], [], m, torch.zeros(1, 2, 23, 4, 19, dtype=torch.int64, device="cuda")),
                 lambda: ops.segment_counts([s], [], m.to(torch.int32))):
        with pytest.raises(DasacError, match="segment_counts"):
            call()


# ---------------------------------------------------------------------------------------------------------------------
# exact workspaces, guarded operands
# ---------------------------------------------------------------------------------------------------------------------
def test_segment_ops_on_exact_workspaces_and_guarded_operands_at_every_phase(monkeypatch, count_cases):
    from dasac_hip import lib as L, ops
    H, W = TH + 1, TW + 1
    scores, labels, gt, _ = count_cases[(H, W)]
    u8 = labels.astype(np.uint8)

    def run(arena):
        d_scores = [arena.place(torch.from_numpy(s)) for s in scores[:2]]
        d_gt, d_i64, d_u8 = arena.place(torch.from_numpy(gt)), arena.place(torch.from_numpy(labels)), arena.place(torch.from_numpy(u8))
        outs = list(ops.label_segments(d_u8, C19, 8)) + list(ops.label_segments(d_i64, C19, 4))
        outs.append(ops.segment_counts(d_scores, [d_i64, d_u8], d_gt))
        outs += [ops.segment_filter(d_u8, 5, C19, 0, 8), ops.segment_filter(d_i64, 5, C19, 255, 4)]
        return outs
    plain = run(Arena(None))
    for phase in range(16):                                                     # uint8 maps at all 16 byte phases
        arena, ws = Arena(phase), ExactWorkspace(slack=0)
        with monkeypatch.context() as mp:
            mp.setattr(L, "workspace", ws)
            mp.setattr(ops, "torch", arena.torch)
            got = run(arena)
        assert ws.check() == 5 and arena.check() > 0
        assert all(arena.owns(t) for t in got)
        for i, (a, b) in enumerate(zip(plain, got)):
            assert bits_equal(a, b), "output {} at phase {} differs from the plain run".format(i, phase)


# ---------------------------------------------------------------------------------------------------------------------
# end to end (the fixtures and the ATen probe of test_gpu_validation.py / test_gpu_boundary.py, restated)
# ---------------------------------------------------------------------------------------------------------------------
SCORE_LAYERS = ["logits_up", "teacher_init", "teacher_refined"]
LAYERS = {"src": ["logits_up"], "tgt": SCORE_LAYERS + ["teacher_labels"]}
STATE_KW = dict(randomize_bn=True, he_init=True, residual_gain=0.25, aspp_gain=0.2)
PLUMBING = {"empty", "empty_like", "empty_strided", "new_empty", "new_empty_strided", "zeros", "zeros_like", "ones", "full", "zero_", "fill_",
            "view", "_unsafe_view", "reshape", "as_strided", "narrow", "slice", "select", "expand", "permute", "transpose", "t", "squeeze",
            "unsqueeze", "flatten", "unflatten", "detach", "detach_", "alias", "clone", "contiguous", "copy_", "_to_copy", "to", "cat",
            "lift_fresh", "_local_scalar_dense", "item", "is_pinned", "_pin_memory", "pin_memory", "record_stream", "set_", "resize_",
            "scalar_tensor", "result_type", "_has_compatible_shallow_copy_type", "is_same_size", "equal", "unbind", "split", "chunk", "stack"}
SMALL = 64          # per-class vectors (19 x 3), losses: arithmetic on these is bookkeeping


class Recorder(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.big = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        name = func.overloadpacket.__name__ if hasattr(func, "overloadpacket") else str(func)
        if name not in PLUMBING:
            sizes = [t.numel() for t in torch.utils._pytree.tree_leaves((args, kwargs, out)) if isinstance(t, torch.Tensor)]
            if sizes and max(sizes) > SMALL:
                self.big.append((name, max(sizes)))
        return out


@pytest.fixture(scope="module")
def g19(golden):
    return golden("g19_validation")


@pytest.fixture(scope="module")
def net19(g19):
    import models as M
    from oracle import nets_ref as N
    from oracle.step_ref import DEFAULT_CFG
    cfg = NS(**dict(DEFAULT_CFG, INIT_MODEL="", OPT_NESTEROV=False))
    net = M.get_model(cfg, 0, num_classes=19, criterion=nn.CrossEntropyLoss(ignore_index=255, reduction="none"))
    net.backbone.load_state_dict(N.resnet101_state(seed=int(g19["student_seed"]), **STATE_KW), strict=True)
    net.slow_net.load_state_dict(N.resnet101_state(seed=int(g19["teacher_seed"]), **STATE_KW), strict=True)
    net.slow_init[0] = True
    net.running_conf.copy_(torch.from_numpy(g19["running_conf"]))
    return net.cuda().train()


def _loader(g19, name):
    """The fixture's loader: 4 batches, the 4th a repeat of the 1st (max_iter = 1 counts 3 of them)."""
    counted, n, t = int(g19["counted"]), int(g19["N"]), int(g19["T"])
    out = []
    for b in range(int(g19["num_batches"])):
        b %= counted
        if name == "src":
            out.append((torch.from_numpy(g19["src%d_x" % b]), torch.from_numpy(g19["src%d_y" % b]).to(torch.int64)))
        else:
            ts = (g19["tgt%d_f1" % b], g19["tgt%d_gt" % b].astype(np.int64), g19["tgt%d_f2" % b], g19["affine"], g19["affine_inv"])
            out.append(tuple(torch.from_numpy(np.ascontiguousarray(a)).view(n, t, *a.shape[1:]) for a in ts))
    return out


@pytest.mark.parametrize("name", ["src", "tgt"])
def test_validation_with_segment_tables_end_to_end(g19, net19, name):
    import driver
    kw = dict(step="source" if name == "src" else "target", group_size=int(g19["T"]), max_iter=int(g19["max_iter"]),
              ignore_classes=[9, 14, 16])
    plain = driver.validation(net19, _loader(g19, name), **kw)
    assert plain.segments == {} and plain.segment_summary is None
    seen = []

    def keep(module, args, output):
        _, outs = output
        seen.append(({layer: outs[layer].cpu().numpy() for layer in LAYERS[name]}, args[1].view(-1, *args[1].shape[-2:]).cpu().numpy().copy()))
    hook = net19.register_forward_hook(keep)
    try:
        res = driver.validation(net19, _loader(g19, name), segment_tables=True, **kw)
    finally:
        hook.remove()
    assert len(seen) == int(g19["counted"])
    # every existing field is the one of the run without the option
    assert list(res.counts) == LAYERS[name] and res.losses == plain.losses
    assert res.checkpoint_score == plain.checkpoint_score and res.mean == plain.mean
    assert res.confusion == {} and res.reliability == {} and res.consistency == {} and res.consistency_summary is None
    assert res.boundary == {} and res.boundary_summary is None
    for layer in LAYERS[name]:
        assert torch.equal(res.counts[layer], plain.counts[layer]), layer
        assert all(torch.equal(a, b) for a, b in zip(res.per_class[layer], plain.per_class[layer])), layer
    # the tables of its own layer maps
    assert list(res.segments) == LAYERS[name]
    for layer in LAYERS[name]:
        want = sum(SR.segment_table(t[layer] if layer == "teacher_labels" else BR.argmax_first(t[layer]), gt, 19, 8) for t, gt in seen)
        got = res.segments[layer]
        assert got.dtype == torch.int64 and not got.is_cuda and tuple(got.shape) == (2, 24, 4, 19)
        assert np.array_equal(got.numpy(), want), layer
        tp, fp, fn = res.counts[layer]
        s = got.sum(1)
        assert torch.equal(s[0, 2], tp) and torch.equal(s[0, 1], tp + fn) and torch.equal(s[1, 1], tp + fp) and torch.equal(s[1, 2], tp)
        assert int(got[:, :, 0].sum()) > 0
    assert list(res.segment_summary) == LAYERS[name] and list(res.segment_summary[LAYERS[name][0]]) == ["< 64", "64-1023", "1024-16383", ">= 16384"]
    assert len(driver.format_segments(res.segment_summary, [str(c) for c in range(19)]).splitlines()) == len(LAYERS[name]) * (1 + 4 + 1 + 19)
    four = driver.validation(net19, _loader(g19, name), segment_tables=True, segment_connectivity=4, **kw)
    layer = LAYERS[name][-1]
    want = sum(SR.segment_table(t[layer] if layer == "teacher_labels" else BR.argmax_first(t[layer]), gt, 19, 4) for t, gt in seen)
    assert np.array_equal(four.segments[layer].numpy(), want)
    if name == "tgt":                                                            # the teacher's pseudo labels without their specks
        labels = torch.from_numpy(seen[0][0]["teacher_labels"]).cuda()
        clean = driver.despeckle(labels, 16)
        assert clean.dtype == labels.dtype and np.array_equal(clean.cpu().numpy(), SR.filter_small(seen[0][0]["teacher_labels"], 16, 19, 255, 8))
        assert torch.equal(driver.despeckle(labels, 1), labels)


@pytest.mark.parametrize("name", ["src", "tgt"])
def test_validation_with_segment_tables_runs_no_aten_arithmetic_on_tensors(g19, net19, name):
    import driver
    kw = dict(step="source" if name == "src" else "target", group_size=int(g19["T"]), max_iter=0, ignore_classes=[9, 14, 16],
              segment_tables=True)
    driver.validation(net19, _loader(g19, name), **kw)                                 # first call: caches
    loader = _loader(g19, name)
    with Recorder() as rec:
        res = driver.validation(net19, loader, **kw)
        torch.cuda.synchronize()
    assert res.checkpoint_score > 0 and int(res.segments["logits_up"].sum()) > 0
    assert not rec.big, sorted(set(rec.big))[:12]
