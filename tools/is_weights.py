"""Importance-sampling weights from a directory of label PNGs -- the reference's tools/compute_IS_weights.py with the
counting on the device.  Usage (GPU box):

    python tools/is_weights.py --labels DIR --ext '*labelIds.png' --out FILE

Decodes with Pillow, uploads batches of equally sized label maps (images of different sizes go in separate launches),
counts with dasac_label_hist, and writes {basename: {label: pixel share}} with sampling.save_weights: plain int / float
entries, readable by torch.load's defaults and by the reference's loader (DATASET.SAMPLE_WEIGHTS).  Every value but 255
is counted.  Inside a training pipeline driver.compute_sample_weights gives the same table straight from the network's
label maps, with no PNGs in between."""
import argparse
import fnmatch
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "da-sac_amd"))
import numpy as np
import torch
from PIL import Image

import sampling
from dasac_hip import ops


def count(labels, ext, out, batch=16):
    if os.path.exists(out):
        raise FileExistsError("File {} already exists".format(out))
    names = sorted(fnmatch.filter(os.listdir(labels), ext))
    print("Found {} masks".format(len(names)))
    table = torch.zeros((len(names), 256), dtype=torch.int64, device="cuda")
    pending = []                                        # (row, uint8 [H,W]): consecutive rows, one size

    def flush():
        if pending:
            maps = torch.from_numpy(np.stack([m for _, m in pending])).cuda()
            ops.label_hist(maps, table[pending[0][0]:pending[0][0] + len(pending)])
        del pending[:]

    for row, name in enumerate(names):
        m = np.array(Image.open(os.path.join(labels, name)))
        if m.dtype != np.uint8 or m.ndim != 2:
            raise ValueError("{}: expected an 8-bit single-channel label image, got {} {}".format(name, m.dtype, m.shape))
        if pending and (pending[0][1].shape != m.shape or len(pending) == batch):
            flush()
        pending.append((row, m))
    flush()
    counts = table.cpu()
    print("\n".join(sampling.format_class_table(counts)))
    sampling.save_weights(out, sampling.weights_from_counts(names, counts))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description="Compute importance sampling weights")
    ap.add_argument("--labels", type=str, required=True, help="Directory with the label PNGs")
    ap.add_argument("--ext", type=str, default="*labelIds.png", help="Filter of the label files")
    ap.add_argument("--out", type=str, required=True, help="Weights file to write")
    a = ap.parse_args()
    count(a.labels, a.ext, a.out)
