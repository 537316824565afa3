"""numpy float64 restatement of the activation table's contract (include/dasac_hip.h, dasac_activation_stats), independent of the
kernel: shared by tests/test_activation_stats_cpu.py and tests/test_gpu_activation_stats.py."""
import numpy as np

COLUMNS = ("sum", "sumsq", "maxabs", "nonfinite", "first_nonfinite", "zeros")


def table(tensors, bounds):
    """tensors: arrays [N, C, ...] (any float dtype; values are taken as they are and widened to float64); bounds: the full tuple
    (0, ..., N).  Returns (table [S, R, 6], abs_sum [S, R], count [S, R]): abs_sum = sum |x| over the finite entries and count the
    elements per (segment, channel), for error bounds."""
    S, R = len(bounds) - 1, sum(t.shape[1] for t in tensors)
    out, abs_sum, count = np.zeros((S, R, 6)), np.zeros((S, R)), np.zeros((S, R))
    row0 = 0
    for t in tensors:
        N, C = t.shape[:2]
        x = np.asarray(t).reshape(N, C, -1)
        HW = x.shape[2]
        for s in range(S):
            lo, hi = bounds[s], bounds[s + 1]
            seg = x[lo:hi].astype(np.float64)                       # [n, C, HW]
            fin = np.isfinite(seg)
            val = np.where(fin, seg, 0.0)
            rows = slice(row0, row0 + C)
            out[s, rows, 0] = val.sum(axis=(0, 2))
            out[s, rows, 1] = (val * val).sum(axis=(0, 2))
            out[s, rows, 2] = np.abs(val).max(axis=(0, 2))
            out[s, rows, 3] = (~fin).sum(axis=(0, 2))
            out[s, rows, 5] = (seg == 0).sum(axis=(0, 2))
            abs_sum[s, rows] = np.abs(val).sum(axis=(0, 2))
            count[s, rows] = (hi - lo) * HW
            for c in range(C):
                bad = np.argwhere(~fin[:, c, :])                    # sorted by (sample, position): the first is the smallest flat index
                if len(bad):
                    n, i = bad[0]
                    out[s, row0 + c, 4] = 1 + ((lo + n) * C + c) * HW + i
        row0 += C
    return out, abs_sum, count


def gap(mu_a, var_a, mu_b, var_b):
    """gap_c of driver.domain_gap_report for one channel."""
    num = (mu_a - mu_b) ** 2 + (np.sqrt(var_a) - np.sqrt(var_b)) ** 2
    return 0.0 if num == 0 else num / max(0.5 * (var_a + var_b), 1e-30)
