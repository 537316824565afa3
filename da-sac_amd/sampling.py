"""Importance-sampled target selection: the weights of the reference's stage 2 and the draw that opens every target sample.

  * `weights_from_counts`  per-image class weights from a [N,256] table of pixel counts (ops.label_hist /
    driver.compute_sample_weights) -- tools/compute_IS_weights.py:58-98 without the PNG round trip;
  * `save_weights` / `load_weights`  the weights file, readable by this project and by the reference's loader;
  * `init_sampling`  the per-class cumulative tables of DataTarget.init_sampling (datasets/dataloader_target.py:151-199);
  * `TargetSampler`  the first three lines of DataTarget.__getitem__ (:264-272).

Host side, float64 / python floats with the reference's order of additions: the tables and the selected indices are
bit-equal to the reference's for the same weights and the same `random` state."""
import bisect
import os

import numpy as np

IGNORE_LABEL = 255              # compute_IS_weights.py:67-68: the one value that is never counted


def weights_from_counts(names, counts):
    """{name: {int label: float}} from `counts[n][v]` = pixels of value v in image n (int [N,256], host array or tensor).
    Only labels that occur in an image appear in its entry, 255 never does, an image with no counted pixel gets {}.
    The value is count / (pixels of that label over all images) in float64, like the reference's `label_stats[label] /=
    pixel_count[label]`.  The reference accumulates the total as a float over the files in listing order; every partial
    sum is an integer below 2^53 and so exact, which makes the total -- and with it every weight -- independent of the
    order of the images."""
    counts = np.asarray(counts.cpu() if hasattr(counts, "cpu") else counts)
    if counts.ndim != 2 or counts.shape[1] != 256 or counts.shape[0] != len(names):
        raise ValueError("counts must be [{},256], got {}".format(len(names), counts.shape))
    if len(set(names)) != len(names):
        raise ValueError("image names must be unique (the weights file is keyed by basename)")
    counts = counts.astype(np.int64)
    totals = counts.sum(axis=0, dtype=np.int64)
    assert int(totals.max(initial=0)) < 2 ** 53, "pixel totals leave the exact range of float64"
    weights = {}
    for n, name in enumerate(names):
        row = counts[n]
        weights[name] = {int(v): float(row[v]) / float(totals[v]) for v in np.flatnonzero(row) if v != IGNORE_LABEL}
    return weights


def class_table(counts):
    """[(label, pixels, images)] over the labels that occur, 255 left out: the reference tool's report."""
    counts = np.asarray(counts.cpu() if hasattr(counts, "cpu") else counts).astype(np.int64)
    return [(int(v), int(counts[:, v].sum()), int((counts[:, v] > 0).sum()))
            for v in range(256) if v != IGNORE_LABEL and counts[:, v].any()]


def format_class_table(counts):
    """The lines compute_IS_weights.py:85-88 prints."""
    return ["Pixel count / # of Images: "] + ["Class {:02d}: {:2.1f} {}".format(v, float(px), im) for v, px, im in class_table(counts)]


def _plain(weights):
    return {str(name): {int(k): float(v) for k, v in stat.items()} for name, stat in weights.items()}


def save_weights(path, weights):
    """torch.save of {name: {int: float}} with plain python keys and values: loads under torch.load's default
    weights_only=True and is what the reference's `torch.load(weights)` + init_sampling read.  Refuses to overwrite an
    existing file, as the reference tool does."""
    import torch
    if os.path.exists(path):
        raise FileExistsError("File {} already exists".format(path))
    torch.save(_plain(weights), path)


def load_weights(path):
    """Reads a file of save_weights, or one the reference tool wrote (numpy-scalar keys and values, which the default
    weights_only=True load refuses), into the plain {name: {int: float}} form."""
    import pickle
    import torch
    try:
        weights = torch.load(path)
    except pickle.UnpicklingError:
        weights = torch.load(path, weights_only=False)
    return _plain(weights)


def init_sampling(num_samples, weights, sample_index, num_classes, ignore_classes=(), prior_weight=0.25):
    """DataTarget.init_sampling (dataloader_target.py:151-199): per class the cumulative selection weights over the
    images, a list [num_classes] of lists [num_samples] of python floats -- a uniform prior of weight `prior_weight` plus
    (1 - prior_weight) x the class's pixel share of every image; uniform for `ignore_classes` (VAL.IGNORE_CLASS) and for
    every class when `weights` is None.  `sample_index`: name -> position in the loader's image list.  The additions run
    in the reference's order (per image in the dict's order, then one sequential prefix sum), so the tables are bit-equal."""
    prior = 1. / num_samples
    ignore_classes = [int(c) for c in ignore_classes]
    if weights is not None:
        assert len(weights) == num_samples, \
            "Loaded weights {} do not match # of loaded images {}".format(len(weights), num_samples)
        groups = [[prior if cid in ignore_classes else prior_weight * prior for _ in range(num_samples)]
                  for cid in range(num_classes)]
        for name, stat in weights.items():
            sample_id = sample_index[name]
            for cid, val in stat.items():
                if not 0 <= cid < num_classes:
                    raise KeyError("weights of {} hold label {}, outside the {} classes (train-id weights are needed)".format(
                        name, cid, num_classes))
                groups[cid][sample_id] += (1. - prior_weight) * val
        for cid in ignore_classes:
            if 0 <= cid < num_classes:
                groups[cid] = [prior for _ in range(num_samples)]
    else:
        groups = [[prior for _ in range(num_samples)] for _ in range(num_classes)]

    for cid, group in enumerate(groups):
        for sample_id in range(1, len(group)):
            group[sample_id] += group[sample_id - 1]
        if not abs(group[-1] - 1.) < 1e-3:
            hint = ""
            if weights is not None and abs(group[-1] - prior_weight) < 1e-3:
                hint = ": class {} occurs in no image of the weights; list it in VAL.IGNORE_CLASS to sample it uniformly".format(cid)
            raise AssertionError("Cumulative weights [{}] do not add up {}{}".format(cid, group[-1], hint))
    return groups


class TargetSampler:
    """The image selection of DataTarget.__getitem__ (dataloader_target.py:264-272): the category is `index % num_classes`,
    the image a draw from that category's cumulative table.  `rng`: a `random.Random` (or the `random` module); one
    `uniform` per select."""

    def __init__(self, tables, rng=None):
        import random
        self.tables = tables
        self.rng = random if rng is None else rng

    @classmethod
    def from_cfg(cls, cfg, names, weights=None, rng=None, num_classes=19):
        """The tables DataTarget(cfg, split, num_classes) builds for the images `names` (basenames, in the loader's order;
        `num_classes` is an argument there too, datasets/__init__.py:17-54).  `weights`: a
        dict, a path, or None for cfg.DATASET.SAMPLE_WEIGHTS; an empty or missing path samples uniformly, with the
        reference's message."""
        if weights is None:
            weights = cfg.DATASET.SAMPLE_WEIGHTS
        if isinstance(weights, (str, bytes, os.PathLike)):
            path, weights = weights, None
            if len(path):
                if os.path.isfile(path):
                    print("Loading sample weights: {}".format(path))
                    weights = load_weights(path)
                else:
                    print("Path to sample weights NOT found: {}".format(path))
        index = {name: i for i, name in enumerate(names)}
        tables = init_sampling(len(names), weights, index, int(num_classes), tuple(cfg.VAL.IGNORE_CLASS),
                               float(cfg.DATASET.SAMPLE_UNIFORM_PRIOR))
        return cls(tables, rng)

    @property
    def num_classes(self):
        return len(self.tables)

    def select(self, index, rng=None):
        rng = self.rng if rng is None else rng
        table = self.tables[index % len(self.tables)]
        r = rng.uniform(0, table[-1])
        # uniform(a, b) may return b, and rounding inside it can land above the last entry; bisect_left then returns
        # num_samples and the reference's list lookup raises IndexError.  Clamped to the last image here.
        return min(bisect.bisect_left(table, r), len(table) - 1)
