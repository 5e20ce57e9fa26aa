"""Test-side helpers of the lineage reports (reina_model_amd/lineage.py): a plain per-agent walker that counts every field of
a report directly, hand-made states, and the invariants that tie a report of a simulated run to the other two reports.

The synthetic states come from tx_util / txlog_util: they are NOT states a simulation could reach.  Never step a day on one."""
import bisect

import numpy as np

from tx_util import assert_words  # noqa: F401  (lineage_util.assert_words: the one of every report util)
from reina_model_amd import lineage as lin
from reina_model_amd import transmission as tx
from reina_model_amd import txlog as txl

PERIODS = ((7, 43), (1, 256), (400, 1), (30, 5))   # (period_days, n_periods)


def walk_report(hot, infector, log, age_start, age_group, period_days, n_periods, max_depth):
    """Every field of a report, counted agent by agent with dicts and plain Python (independent of report_numpy)"""
    n = len(hot)
    hot = [int(x) for x in np.asarray(hot, dtype=np.uint32)]
    src = [int(x) for x in np.asarray(infector, dtype=np.int32)]
    log = [int(x) for x in np.asarray(log, dtype=np.uint32)]
    starts = [int(x) for x in age_start]
    nr_ages = len(age_group)
    P, Q = n_periods, n_periods + 1
    group = lambda i: int(age_group[min(max(bisect.bisect_right(starts[:nr_ages + 1], i) - 1, 0), nr_ages - 1)])

    def pc(i):
        d = log[i] & 0xFFFF
        if d in (txl.NONE, txl.BEFORE) or d // period_days >= P:
            return P
        return d // period_days

    rounds = tx.rounds_for(max_depth)
    reach = (1 << rounds) - 1      # after r rounds every agent within 2^r - 1 links of its root has found it
    seed = np.zeros((Q, 4), dtype=np.uint64)
    tree_sizes = np.zeros((Q, 33), dtype=np.uint64)
    cohort = np.zeros((Q, 16, 2), dtype=np.uint64)
    lineage = np.zeros((Q, Q), dtype=np.uint64)
    mixing_t = np.zeros((Q, 16, 16), dtype=np.uint64)
    mixing_c = np.zeros((Q, 16, 16), dtype=np.uint64)
    sc = {name: 0 for name in lin.SCALAR_NAMES}
    sc['rounds'] = rounds
    link = {}
    for i in range(n):
        st = hot[i] & 7
        if st == 0:
            continue
        sc['infected'] += 1
        cohort[pc(i), group(i), 0] += 1
        if st >= 5:
            cohort[pc(i), group(i), 1] += 1
        if pc(i) == P:
            sc['undated'] += 1
        s = src[i]
        if s == -1:
            sc['roots'] += 1
            link[i] = None
        elif 0 <= s < n and s != i and hot[s] & 7 != 0:
            sc['links'] += 1
            link[i] = s
            mixing_t[pc(i), group(s), group(i)] += 1
            mixing_c[pc(s), group(s), group(i)] += 1
        else:
            sc['bad_links'] += 1
            link[i] = None
    members = {}   # head of a tree -> its converged agents
    for i in link:
        a, steps = i, 0
        while link[a] is not None and steps < reach:
            a = link[a]
            steps += 1
        if link[a] is not None:        # deeper than the rounds reach, or on a cycle
            sc['unconverged'] += 1
            continue
        members.setdefault(a, []).append(i)
    largest, lroot = 0, None
    for head in sorted(members):
        agents = members[head]
        alive = [i for i in agents if 1 <= hot[i] & 7 <= 4]
        c = pc(head)
        seed[c, 0] += 1
        seed[c, 2] += len(agents)
        seed[c, 3] += len(alive)
        if alive:
            seed[c, 1] += 1
            sc['alive_trees'] += 1
        sc['trees'] += 1
        sc['alive_agents'] += len(alive)
        tree_sizes[c, len(agents).bit_length() - 1] += 1
        for i in agents:
            lineage[c, pc(i)] += 1
        if len(agents) > largest:
            largest, lroot = len(agents), head
    sc.update(largest_tree=largest, largest_root=(1 << 64) - 1 if lroot is None else lroot,
              largest_key=0 if lroot is None else largest << 32 | (~lroot & 0xFFFFFFFF))
    w = np.concatenate([np.array([sc[name] for name in lin.SCALAR_NAMES] + [0] * (lin.S_NR - len(lin.SCALAR_NAMES)), dtype=np.uint64),
                        seed.ravel(), tree_sizes.ravel(), cohort.ravel(), lineage.ravel(), mixing_t.ravel(), mixing_c.ravel()])
    assert len(w) == lin.report_words(P)
    return w


def cycle_state():
    """(hot, infector, n_infected, log): a 2-cycle of links 3 <-> 5 with agent 7 hanging on it, beside a root 1 with a child 2"""
    n = 10
    hot = np.zeros(n, dtype=np.uint32)
    inf = np.full(n, -1, dtype=np.int32)
    hot[[1, 2, 3, 5, 7]] = (5, 2, 1, 2, 3)
    inf[2], inf[3], inf[5], inf[7] = 1, 5, 3, 3
    log = np.full(n, txl.NONE << 16 | txl.NONE, dtype=np.uint32)
    log[[1, 2, 3, 5, 7]] = [txl.NONE << 16 | d for d in (0, 9, 3, 4, 12)]
    return hot, inf, np.zeros(n, dtype=np.int32), log


def bin_by_period(per_day, period_days, n_periods):
    """a per-day array summed into the periods [0, n_periods) (every day must lie in them)"""
    per_day = np.asarray(per_day).astype(np.int64)
    assert len(per_day) <= period_days * n_periods
    out = np.zeros(n_periods, dtype=np.int64)
    np.add.at(out, np.arange(len(per_day)) // period_days, per_day)
    return out


def assert_run_invariants(r, tree, log_report):
    """what ties the lineage report `r` of a simulated run to the tree report and the log report of the same state (all of
    the run's days inside the report's periods, the log kept from day 0)"""
    P = r.n_periods
    assert r.unconverged == 0 and r.bad_links == 0
    assert int(r.seed[:, 2].sum()) == int(r.lineage.sum()) == r.infected == tree.n_infected_agents
    assert np.array_equal(r.lineage.sum(axis=1), r.seed[:, 2])
    assert np.array_equal(r.lineage.sum(axis=0), r.cohort[..., 0].sum(axis=1))
    assert int(r.mixing_t.sum()) == int(r.mixing_c.sum()) == r.links == tree.n_linked
    assert np.array_equal(r.mixing_t.sum(axis=0), tree.matrix.sum(axis=0))
    assert np.array_equal(r.tree_sizes.sum(axis=0), tree.clusters)
    assert r.largest_tree == tree.largest_cluster and r.largest_root == tree.largest_root
    assert r.roots == r.trees == tree.n_roots == int(r.seed[:, 0].sum())
    assert int(r.seed[:, 1].sum()) == r.alive_trees and int(r.seed[:, 3].sum()) == r.alive_agents
    got = r.cohort[..., 0].sum(axis=1).astype(np.int64)
    assert np.array_equal(got[:P], bin_by_period(log_report.incidence.sum(axis=(1, 2)), r.period_days, P))
    assert log_report.out_of_range == 0 and int(got[P]) == r.undated == log_report.before
    assert np.array_equal(r.mixing_c.sum(axis=(1, 2)).astype(np.int64)[:P],
                          bin_by_period(log_report.cohort[..., 1].sum(axis=1), r.period_days, P))
    assert 0 < r.alive_trees < r.trees
