"""Test-side helpers of the logged particle filter (tests/test_filter_log.py, tests/test_filter_log_gpu.py)."""
import numpy as np

CLONE_DAY = 60          # the day of the clone tests: on oracle B all four classes of agents occur between seeds 1 and 2


def classes(dst_hot, src_hot):
    """the agents recorded in both members, in src only, in dst only, in neither"""
    d, s = np.asarray(dst_hot) != 0, np.asarray(src_hot) != 0
    return int((d & s).sum()), int((~d & s).sum()), int((d & ~s).sum()), int((~d & ~s).sum())


def incidence_by_day(report):
    """infections by date of infection of a txlog.LogReport, summed over variants and groups: int64 [n_days]"""
    return report.incidence.sum(axis=(1, 2), dtype=np.uint64).astype(np.int64)
