"""Golden vectors of the importance-sampling weights and the target image selection (g18).  Runs ONLY in the build container
(needs the reference):

    cd <repo> && python -B tests/golden/make_goldens_sampling.py

The reference's own tool (tools/compute_IS_weights.py: `count`) is run on a directory of small synthetic label PNGs, its
DataTarget.init_sampling on the weights it wrote (with VAL.IGNORE_CLASS empty and with SYNTHIA's 9,14,16), and the three
selection lines of DataTarget.__getitem__ under seeded python `random`.  The tool uses `np.float`, which NumPy >= 1.24 no
longer has: the alias is restored before the tool is loaded.  Only data goes into the file.
"""
import bisect
import importlib.util
import os
import random
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens_crops  # noqa: E402,F401  (imports the reference, registers the torchvision stand-in modules)
from ref_import import REFERENCE_ROOT  # noqa: E402

from PIL import Image  # noqa: E402

np.float = float
_spec = importlib.util.spec_from_file_location("ref_compute_is_weights", os.path.join(REFERENCE_ROOT, "tools", "compute_IS_weights.py"))
ref_tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref_tool)
from datasets.dataloader_target import DataTarget  # noqa: E402

N, NUM_CLASSES, PRIOR = 12, 19, 0.25
IGNORE_SYNTHIA = [9, 14, 16]            # launch/train.sh:41
ALL_IGNORE = 3                          # the image that is entirely 255


def label_maps():
    """12 blocky label maps of different sizes with skewed class mixes, ~10 % of 255, one image entirely 255; every class
    0..18 occurs in at least one image (the reference asserts on a class that occurs nowhere unless it is ignored)."""
    rng = np.random.RandomState(18)
    maps = []
    for i in range(N):
        h, w = 40 + 4 * ((i * 7) % 11), 64 + 5 * ((i * 5) % 12)
        mix = rng.dirichlet(np.full(NUM_CLASSES, 0.3))
        coarse = rng.choice(NUM_CLASSES, size=((h + 7) // 8, (w + 7) // 8), p=mix).astype(np.uint8)
        lab = np.kron(coarse, np.ones((8, 8), np.uint8))[:h, :w].copy()
        noise = rng.rand(h, w) < 0.05                     # a few single pixels of other classes
        lab[noise] = rng.choice(NUM_CLASSES, size=int(noise.sum()), p=mix)
        lab[rng.rand((h + 3) // 4, (w + 3) // 4).repeat(4, 0).repeat(4, 1)[:h, :w] < 0.1] = 255
        lab[0, :2] = [(2 * i) % NUM_CLASSES, (2 * i + 1) % NUM_CLASSES]        # 24 slots cover the 19 classes
        if i == ALL_IGNORE:
            lab[:] = 255
        maps.append(lab)
    present = set(np.unique(np.concatenate([m.ravel() for m in maps]))) - {255}
    assert present == set(range(NUM_CLASSES)), sorted(present)
    return maps


def main():
    maps = label_maps()
    names = ["target_{:03d}_gtFine_labelIds.png".format(i) for i in range(N)]
    with tempfile.TemporaryDirectory() as d:
        for name, lab in zip(names, maps):
            Image.fromarray(lab).save(os.path.join(d, name))
        out = os.path.join(d, "weights.data")
        ref_tool.count(d, "*labelIds.png", out)
        loaded = torch.load(out, weights_only=False)
    assert set(loaded) == set(names) and loaded[names[ALL_IGNORE]] == {}
    order = list(loaded)                                  # the file's (= the tool's listing) order: init_sampling iterates it

    weights = np.zeros((N, 256), np.float64)
    present = np.zeros((N, 256), np.uint8)
    for n, name in enumerate(names):
        for label, val in loaded[name].items():
            weights[n, int(label)] = float(val)
            present[n, int(label)] = 1

    arrays = {"names": np.array(names), "file_order": np.array([names.index(o) for o in order], np.int32),
              "weights": weights, "present": present, "prior_weight": np.float64(PRIOR),
              "ignore_synthia": np.array(IGNORE_SYNTHIA, np.int32), "sizes": np.array([m.shape for m in maps], np.int32)}
    for n, lab in enumerate(maps):
        arrays["labels%d" % n] = lab

    sample_index = {name: i for i, name in enumerate(names)}
    for tag, ignore in (("none", []), ("synthia", IGNORE_SYNTHIA)):
        self = types.SimpleNamespace(num_classes=NUM_CLASSES, sample_index=sample_index,
                                     cfg=types.SimpleNamespace(VAL=types.SimpleNamespace(IGNORE_CLASS=ignore)))
        groups = DataTarget.init_sampling(self, N, loaded, prior_weight=PRIOR)
        table = np.array([[float(x) for x in groups[cid]] for cid in range(NUM_CLASSES)], np.float64)
        arrays["tables_" + tag] = table
        seeds, picks = [], []
        for seed in range(8):
            random.seed(seed)
            row = []
            for index in range(64):                       # dataloader_target.py:266-272, executed on the reference's tables
                cum = groups[index % len(groups)]
                row.append(bisect.bisect_left(cum, random.uniform(0, cum[-1])))
            seeds.append(seed)
            picks.append(row)
        arrays["select_seeds"] = np.array(seeds, np.int32)
        arrays["select_" + tag] = np.array(picks, np.int32)

    self = types.SimpleNamespace(num_classes=NUM_CLASSES, sample_index=sample_index,
                                 cfg=types.SimpleNamespace(VAL=types.SimpleNamespace(IGNORE_CLASS=[])))
    groups = DataTarget.init_sampling(self, N, None, prior_weight=PRIOR)
    arrays["tables_uniform"] = np.array([[float(x) for x in groups[cid]] for cid in range(NUM_CLASSES)], np.float64)

    path = os.path.join(HERE, "g18_is_sampling.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
