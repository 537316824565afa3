"""The bits of the Winograd paths, F(2x2,3x3) and F(4x4,3x3), on a fixed list of small cases: every transform kernel through its C
entry point, and the whole operations through ops (the Python plumbing: workspace carving, the point-sum index, the batched launch).

    python tools/winograd_bits.py --record PATH     write the results to an .npz
    python tools/winograd_bits.py --compare PATH    run the cases again and print, per result, differing elements and largest difference

Inputs come from a closed-form integer hash of the element index evaluated in numpy (no library random generator: the same numbers
everywhere), scaled to float32 in [-1, 1) with all 24 mantissa bits in use, so that every transform rounds.  A result of at most
16384 elements is stored as its int32 bit pattern, a larger one as the SHA-256 of its bytes.  tests/golden/g22_winograd_bits.npz was
recorded once, from the commit before the two forms were folded into one kernel family, and tests/test_gpu_winograd_bits.py requires
equality of every bit with it: a refactor of these paths must not move a bit, so the file is not re-recorded for one."""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "da-sac_amd"))

MAX_STORED = 16384
GEOMS = [(2, 3, 9, 11, 2),      # q % TM == 0 with r > 0 on H for TM = 2 and TM = 4: the leftover tiles exist
         (1, 2, 7, 5, 4),       # one sample per phase, mostly overhang, empty phases
         (2, 1, 6, 10, 1),      # d = 1, r = 0
         (3, 2, 41, 43, 1)]     # more than 256 tiles in both forms (a second block); F(4x4): 363 real tiles, T = 364, one padding tile
FILTERS = [(5, 7), (130, 20)]   # (Cout, Cin): M and K padding
FORMS = {"f2": (16, "winograd"), "f4": (36, "winograd4")}      # points, name stem of the C entry points and of the ops functions
# wgrad_finish, M = C = 128: the smallest T the batched contraction takes (one split), and the smallest with more than 4 splits
FINISH_T = [(4, 1), (1028, 5)]


def _hash(n, salt):
    i = np.arange(n, dtype=np.uint64)
    v = (i * np.uint64(2654435761) + np.uint64(salt)) & np.uint64(0xFFFFFFFF)
    v ^= v >> np.uint64(15)
    v = (v * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    v ^= v >> np.uint64(13)
    return v


def values(shape, salt, dev):
    """float32 in [-1, 1): (24 bits of the hash - 2^23) / 2^23, exact in float32."""
    n = int(np.prod(shape))
    v = (_hash(n, salt) >> np.uint64(8)).astype(np.int64) - (1 << 23)
    return torch.from_numpy((v.astype(np.float64) / (1 << 23)).astype(np.float32).reshape(shape)).to(dev)


def words(n, salt, dev):
    return torch.from_numpy(_hash(n, salt).astype(np.uint32).view(np.int32).copy()).to(dev)


def run_cases():
    """name -> int32 tensor on the CPU (the bit pattern of a result) or a string (an error's text)."""
    from dasac_hip import lib as L
    from dasac_hip import ops
    lib = L.load()
    dev = torch.device("cuda", 0)
    res = {}

    def nan(*shape):
        return torch.full(shape, float("nan"), device=dev)

    def keep(name, t):
        res[name] = t.contiguous().view(torch.int32).cpu()

    for form, (P, stem) in FORMS.items():
        c = lambda fn: getattr(lib, "dasac_{}_{}".format(stem, fn))
        conv, wgrad = getattr(ops, stem + "_conv"), getattr(ops, stem + "_wgrad")
        filt, output = getattr(ops, stem + "_filter"), getattr(ops, stem + "_output")
        for gi, (N, C, H, W, d) in enumerate(GEOMS):
            tag = "{}/{}x{}x{}x{}_d{}".format(form, N, C, H, W, d)
            T = c("tiles")(N, H, W, d)
            x = values((N, C, H, W), 101 + gi, dev)
            v = nan(P, C, T)
            L.check(c("input")(x.data_ptr(), N, C, H, W, d, v.data_ptr(), v.numel() * 4, L.stream_ptr()), "input")
            keep(tag + "/input", v)
            v = nan(P, C, T)
            L.check(c("grad_input")(x.data_ptr(), N, C, H, W, d, v.data_ptr(), v.numel() * 4, L.stream_ptr()), "grad_input")
            keep(tag + "/grad", v)
            # output transforms of Y [P, 3, T]: plain; shift + ReLU + recorded bits; masked
            M = 3
            y, shift = values((P, M, T), 201 + gi, dev), values((M,), 301 + gi, dev)
            keep(tag + "/output_plain", output(y, nan(N, M, H, W), d))
            bits = ops.ReluBits(N, M, H, W, dev)
            bits.words.fill_(-1)
            keep(tag + "/output_relu", output(y, nan(N, M, H, W), d, shift, True, bits_out=bits))
            keep(tag + "/output_relu_bits", bits.words)
            mask = ops.ReluBits(N, M, H, W, dev)
            mask.words.copy_(words(mask.words.numel(), 401 + gi, dev))
            keep(tag + "/output_masked", output(y, nan(N, M, H, W), d, mask_bits=mask))
        for fi, (Cout, Cin) in enumerate(FILTERS):
            w, scale = values((Cout, Cin, 3, 3), 501 + fi, dev), values((Cout,), 601 + fi, dev)
            spec = ops.ConvSpec(Cin, Cout, [(3, 3, 1, 1)])
            for transposed in (False, True):
                for sc in (None, scale):
                    u = filt(spec, w, transposed, sc, out=None)
                    u.fill_(float("nan"))
                    u = filt(spec, w, transposed, sc, out=u)
                    Mr, Kr = (Cin, Cout) if transposed else (Cout, Cin)
                    packed = u.view(P, -1, u.shape[2], 4)       # [P, Kpad/4, Mpad, 4], k = 4 * quad + lane: the K and M padding are zeros
                    k = torch.arange(u.shape[1], device=dev).view(-1, 1, 4).expand(packed.shape[1:])
                    assert not bool(packed[:, :, Mr:, :].any()) and not bool(packed[:, k >= Kr].any())
                    keep("{}/filter_{}x{}{}{}".format(form, Cout, Cin, "_T" if transposed else "", "_scaled" if sc is not None else ""), u)
        M = C = 128
        w, scale = values((M, C, 3, 3), 701, dev), values((M,), 702, dev)
        for T, want_splits in FINISH_T:
            splits = lib.dasac_conv_wgrad_batched_splits(P, M, C, T)
            assert splits == want_splits, (P, T, splits)
            ws = values((lib.dasac_conv_wgrad_batched_workspace(P, M, C, T) // 4,), 703 + T, dev)
            for full in (False, True):
                dw, dot, sums = nan(M, C, 3, 3), nan(C // 64, M), nan(M)
                L.check(c("wgrad_finish")(ws.data_ptr(), ws.numel() * 4, M, C, T, w.data_ptr(), L.ptr(scale if full else None), dw.data_ptr(),
                                          L.ptr(dot if full else None), L.ptr(sums if full else None), L.stream_ptr()), "wgrad_finish")
                tag = "{}/finish_T{}{}".format(form, T, "_scale_dot_sums" if full else "")
                keep(tag + "/dw", dw)
                if full:
                    keep(tag + "/dot", dot)
                    keep(tag + "/sum_dz", sums)
        # whole operations: C = M = 128, H = W = 17, d = 2, two samples (and four for the weight gradient: F(2x2) has 162 tiles at two
        # samples, no multiple of 4, so its batched contraction refuses them -- the refusal's text is the pinned result there)
        H = W = 17
        d = 2
        spec = ops.ConvSpec(C, M, [(3, 3, d, d)])
        shift = values((M,), 801, dev)
        for N in (2, 4):
            x, dz = values((N, C, H, W), 802 + N, dev), values((N, M, H, W), 803 + N, dev)
            tag = "{}/ops_N{}".format(form, N)
            if N == 2:
                bits = ops.ReluBits(N, M, H, W, dev)
                bits.words.fill_(-1)
                keep(tag + "/forward", conv(x, filt(spec, w, False, scale), nan(N, M, H, W), d, shift, True, bits_out=bits))
                keep(tag + "/forward_bits", bits.words)
                mask = ops.ReluBits(N, C, H, W, dev)
                mask.words.copy_(words(mask.words.numel(), 804, dev))
                keep(tag + "/dgrad_masked", conv(dz, filt(spec, w, True, scale), nan(N, C, H, W), d, mask_bits=mask))
            dot, sums = nan(ops.dot_rows(spec), M), nan(M)
            try:
                dw = wgrad(spec, dz, x, w, scale=scale, dot=dot, sum_dz=sums, out=nan(M, C, 3, 3))
            except L.DasacError as e:
                res[tag + "/wgrad_refused"] = str(e)
                continue
            keep(tag + "/wgrad_dw", dw)
            keep(tag + "/wgrad_dot", dot)
            keep(tag + "/wgrad_sum_dz", sums)
    torch.cuda.synchronize()
    return res


def stored(value):
    """What the .npz holds for a result: the int32 array, the SHA-256 of a large one's bytes, or an error's text."""
    if isinstance(value, str):
        return np.array("error:" + value)
    a = value.numpy()
    return a if a.size <= MAX_STORED else np.array("sha256:" + hashlib.sha256(a.tobytes()).hexdigest())


def compare(res, golden):
    """[(name, differing elements or None for a hashed / textual result, largest difference, equal?)] over the golden file's entries;
    a result the run did not produce counts as different."""
    rows = []
    for name in golden.files:
        want = golden[name]
        if name not in res:
            rows.append((name, None, float("nan"), False))
            continue
        got = stored(res[name])
        if want.dtype.kind == "U" or got.dtype.kind == "U":
            rows.append((name, None, float("nan"), got.dtype == want.dtype and str(got) == str(want)))
            continue
        same_shape = got.shape == want.shape
        ndiff = int((got != want).sum()) if same_shape else want.size
        big = 0.0
        if ndiff and same_shape and not name.endswith("bits"):
            big = float(np.nanmax(np.abs(got.view(np.float32).astype(np.float64) - want.view(np.float32).astype(np.float64))))
        rows.append((name, ndiff, big, ndiff == 0))
    rows += [(name, None, float("nan"), False) for name in res if name not in golden.files]
    return rows


def main():
    ap = argparse.ArgumentParser()
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--record", metavar="PATH")
    g.add_argument("--compare", metavar="PATH")
    args = ap.parse_args()
    res = run_cases()
    if args.record:
        np.savez_compressed(args.record, **{k: stored(v) for k, v in res.items()})
        print("recorded {} results to {} ({} bytes)".format(len(res), args.record, os.path.getsize(args.record)))
        return 0
    rows = compare(res, np.load(args.compare))
    for name, ndiff, big, ok in rows:
        print("{:<48s} {}".format(name, "equal" if ok else "DIFFERS: {} elements, largest difference {:.3e}".format(
            "hash / text" if ndiff is None else ndiff, big)))
    bad = sum(not r[3] for r in rows)
    print("{} of {} results differ".format(bad, len(rows)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
