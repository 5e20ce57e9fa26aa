"""Test-side definitions of the regime tests (reina_model_amd/regime.py): the scenario, the policy, the labellings and a plain
per-agent walker that counts every field of a report directly -- shared by the CPU tests (tests/test_regime.py, oracle B) and
the GPU tests (tests/test_regime_gpu.py) in ONE place.  tests/test_regime.py asserts on oracle B that these inputs exercise what
the GPU tests need: every level reached, escalations and relaxations on differing days, links that cross a change of level."""
import bisect

import numpy as np

import policy_util as pu
from reina_model_amd import engine as eng
from reina_model_amd import policy as pol
from reina_model_amd import regime as rgm
from reina_model_amd import reports
from reina_model_amd import txlog as txl

DAYS = 160
SEEDS = (1, 2, 3)
STRETCHES = (60, 100)              # a run in two pieces
LATE_LOG_DAY = 40                  # a log begun mid-run
N_DAYS_CASES = (1, 37, eng.MAX_DAYS)
SMALL_POPULATIONS = (1024, 1025, 1535)   # 2 tiles, 2 tiles + 1 agent, 3 tiles - 1 agent
SMALL_DAYS = 60


def scenario():
    """policy_util.mini_scenario(): 19 997 agents -- 39 tiles and 29 agents, a ragged last tile"""
    return pu.mini_scenario()


def regime_policy():
    """mini_policy's levels under thresholds every seed of SEEDS crosses both ways (mini_policy's own sit on the knife edge on
    purpose: they do not trigger for seeds 1 and 2)"""
    levels = pu.mini_policy().levels
    return pol.Policy(pol.Signal('all_detected', 'increment', 7), levels=levels, up=[60, 200], down=[30, 120], review_every=1, min_days=5)


def small_ages(total):
    """age_counts of a population of exactly `total` agents over 100 ages"""
    base, extra = divmod(int(total), 100)
    return [base + (1 if a < extra else 0) for a in range(100)]


def labellings(levels, n_days=DAYS):
    """{name: (labels, n_days)}: the labellings every report test runs -- the levels themselves, d % 8, the levels with every
    fifth day unlabelled, and n_days = 1, 37 and MAX_DAYS (labels beyond the run: none)"""
    levels = np.asarray(levels, dtype=np.uint8)
    days = np.arange(n_days)
    out = dict(levels=(levels[:n_days], n_days), modulo=((days % 8).astype(np.uint8), n_days),
               fifth=(np.where(days % 5 == 4, rgm.NO_REGIME, levels[:n_days]).astype(np.uint8), n_days))
    for n in N_DAYS_CASES:
        lab = np.full(n, rgm.NO_REGIME, dtype=np.uint8)
        k = min(n, len(levels))
        lab[:k] = levels[:k]
        out['n_days_%d' % n] = (lab, n)
    return out


def state(ctx):
    """(hot, infector, n_infected, log words) of a logged Context, host copies"""
    hot, infector, n_infected, _ = reports.host_state(ctx.engine)
    return hot.copy(), infector.view(np.int32).copy(), n_infected.view(np.int32).copy(), ctx.transmission_log.words()


def spec_report(ctx, labels, n_days, groups=None):
    """regime.report_numpy of a Context's state and log"""
    return rgm.report_numpy(*state(ctx), ctx.age_start, ctx._tx_groups(groups)[0], labels, n_days)


def walk_report(hot, infector, n_infected, log, age_start, age_group, labels, n_days):
    """Every word of a report, counted agent by agent in plain Python (independent of report_numpy and of reports.links)"""
    n = len(hot)
    hot = [int(x) for x in np.asarray(hot, dtype=np.uint32)]
    src = [int(x) for x in np.asarray(infector, dtype=np.int32)]
    cnt = [int(x) for x in np.asarray(n_infected, dtype=np.int32).view(np.uint32)]
    log = [int(x) for x in np.asarray(log, dtype=np.uint32)]
    labels = [int(x) for x in labels]
    starts = [int(x) for x in age_start]
    nr_ages = len(age_group)
    age = lambda i: min(max(bisect.bisect_right(starts[:nr_ages + 1], i) - 1, 0), nr_ages - 1)
    known = lambda x: x not in (txl.NONE, txl.BEFORE)
    clip = lambda x, bins: min(max(x, 0), bins - 1)

    def slot(d):
        if known(d) and d < n_days and labels[d] < 8:
            return labels[d]
        return 8

    days = np.zeros(9, dtype=np.uint64)
    infections = np.zeros((9, 4, 16), dtype=np.uint64)
    cohort = np.zeros((9, 4, 3), dtype=np.uint64)
    offspring = np.zeros((9, 32), dtype=np.uint64)
    gen = np.zeros((9, 64), dtype=np.uint64)
    ser = np.zeros((9, 128), dtype=np.uint64)
    tost = np.zeros((9, 64), dtype=np.uint64)
    phase = np.zeros((9, 4), dtype=np.uint64)
    crossing = np.zeros((9, 9), dtype=np.uint64)
    mixing = np.zeros((9, 16, 16), dtype=np.uint64)
    sc = {name: 0 for name in rgm.SCALAR_NAMES}
    for d in range(n_days):
        days[slot(d)] += 1
    for i in range(n):
        h = hot[i]
        if h & 7 == 0:
            continue
        v = (h >> 8) & 3
        t, o = log[i] & 0xFFFF, log[i] >> 16
        r, g = slot(t), age_group[age(i)]
        sc['infected'] += 1
        if known(t):
            sc['dated'] += 1
            if t < n_days:
                sc['in_range'] += 1
                if r == 8:
                    sc['unlabelled'] += 1
        infections[r, v, g] += 1
        cohort[r, v, 0] += 1
        cohort[r, v, 1] += cnt[i]
        if h & 7 >= 5:
            cohort[r, v, 2] += 1
            offspring[r, min(cnt[i], 31)] += 1
        s = src[i]
        if s == -1:
            continue
        if not (0 <= s < n and s != i and hot[s] & 7 != 0):
            sc['bad_links'] += 1
            continue
        sc['links'] += 1
        ts, os_ = log[s] & 0xFFFF, log[s] >> 16
        rs = slot(ts)
        if known(t) and known(ts):
            sc['links_dated'] += 1
            gen[r, clip(t - ts, 64)] += 1
        if known(o) and known(os_):
            ser[r, clip(o - os_ + 32, 128)] += 1
        if known(t) and known(os_):
            tost[r, clip(t - os_ + 24, 64)] += 1
            phase[r, 0 if t < os_ else 1] += 1
        elif known(t) and os_ == txl.NONE:
            phase[r, 2] += 1
        else:
            phase[r, 3] += 1
        crossing[rs, r] += 1
        if r < 8 and rs < 8 and r != rs:
            sc['links_crossing'] += 1
        mixing[r, age_group[age(s)], g] += 1
    w = np.concatenate([days, infections.ravel(), cohort.ravel(), offspring.ravel(), gen.ravel(), ser.ravel(), tost.ravel(), phase.ravel(),
                        crossing.ravel(), mixing.ravel(), np.array([sc[name] for name in rgm.SCALAR_NAMES], dtype=np.uint64)])
    assert len(w) == rgm.REPORT_WORDS
    return w


def assert_words(got, want, what):
    bad = np.flatnonzero(np.asarray(got, dtype=np.uint64) != np.asarray(want, dtype=np.uint64))
    assert len(bad) == 0, '%s: %d words differ, first at %d (%d != %d)' % (what, len(bad), bad[0], int(got[bad[0]]), int(want[bad[0]]))


def assert_ties(reg, log):
    """a RegimeReport and the LogReport of the same state, both with n_days past the last day and the same labels: what is a sum
    by date agrees after the join on the host, and what is per link agrees summed over the slots"""
    labels = np.asarray(reg.labels, dtype=np.int64)
    assert reg.n_days == log.n_days and log.out_of_range == 0
    for r in range(rgm.SLOTS):
        days = np.flatnonzero((labels == r) if r < 8 else (labels >= 8))
        assert int(reg.days[r]) == len(days)
        want = log.cohort[days].sum(axis=0, dtype=np.uint64)
        if r < 8:
            assert np.array_equal(reg.cohort[r], want), 'cohort of regime %d' % r
        else:   # (slot 8 also holds the agents infected before the log began: they are in no cohort by day)
            assert int(reg.cohort[8, :, 0].sum()) - int(want[:, 0].sum()) == reg.infected - reg.dated, 'cohort without a regime'
    assert int(reg.cohort[:, :, 0].sum()) == reg.infected
    for name in ('generation', 'serial', 'tost', 'link_phase'):
        assert np.array_equal(getattr(reg, name).sum(axis=0, dtype=np.uint64), getattr(log, name).sum(axis=0, dtype=np.uint64)), name
    assert int(reg.crossing.sum()) == reg.links == log.links == int(reg.mixing.sum())
    assert int(reg.infections[:8].sum()) == reg.in_range - reg.unlabelled
    assert (reg.infected, reg.dated, reg.links_dated, reg.bad_links) == (log.infected, log.dated, log.links_dated, log.bad_links)
