"""Stored bits of the single-source label map (g21).  Runs ONLY on the MI355X, once, against the library of the commit BEFORE
dasac_infer_labels and dasac_infer_fuse became one kernel (ca881c4: `infer_labels<CT>` of csrc/head.hip), built apart and named
by DASAC_LIB:

    cd <repo> && DASAC_LIB=<that commit's libdasac_hip.so> python -B tests/golden/make_goldens_infer_bits.py [out.npz]

The inputs are not stored: they are the seeded CPU draws `_logits()` of tests/test_gpu_infer_fused.py, picked by its
BITS_INPUTS.  Stored per input i: shape_i (of the logits), labels_i (uint8 [B,H,W]) and conf_i (float32 [B,H,W]) of
`ops.infer_labels(x, size, want_conf=True)`.  test_infer_fuse_exact_identities holds both entries to them bit for bit."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "da-sac_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    import test_gpu_infer_fused as T
    from dasac_hip import ops
    from dasac_hip import lib as L
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "g21_infer_labels_bits.npz")
    arrays = {}
    for i, (case_index, source) in enumerate(T.BITS_INPUTS):
        x, size = T._logits()[case_index][source], (T.CASE1, T.CASE2)[case_index]["size"]
        labels, conf = ops.infer_labels(x.cuda(), size, want_conf=True)
        arrays["shape_%d" % i] = np.array(x.shape, dtype=np.int64)
        arrays["labels_%d" % i] = labels.cpu().numpy()
        arrays["conf_%d" % i] = conf.cpu().numpy()
        print("input {}: {} -> {}, {} classes present, conf in [{:.4f}, {:.4f}]".format(
            i, tuple(x.shape), size, len(np.unique(arrays["labels_%d" % i])), float(conf.min()), float(conf.max())))
    np.savez_compressed(out, **arrays)
    print("library {}\nwrote {} ({} bytes)".format(L.LIB_PATH, out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
