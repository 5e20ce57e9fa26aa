"""Test-side helpers of the particle filter (reina_model_amd/filtering.py): the continuation check of the clone, observations
from a twin run, the comparison of engine states."""
import copy
from datetime import date, timedelta

import numpy as np

from reina_model_amd import engine as eng
from reina_model_amd import ensemble, filtering, simulation
from reina_model_amd.variables import VARIABLE_DEFAULTS


def small_scenario(n=20000):
    from reina_model_amd import datasets
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    v.update(hospital_beds=12, icu_units=2)
    return v, datasets.scaled_population(n)


def totals(hist, attr):
    """[..., days]: the sum over ages of one counter of history rows"""
    ci = eng.C_NAMES.index(attr)
    return np.asarray(hist)[..., ci * eng.MAX_AGES:(ci + 1) * eng.MAX_AGES].astype(np.int64).sum(axis=-1)


def observations(hist, start_date, rows, streams=('all_detected', 'in_ward')):
    """a DataFrame indexed by date: the streams' totals of history rows `rows` (what get_detected_cases looks like)"""
    import pandas as pd
    d0 = date.fromisoformat(start_date)
    rows = list(rows)
    return pd.DataFrame({s: totals(hist, s)[rows] for s in streams}, index=[d0 + timedelta(days=int(r)) for r in rows])


def carried(engine):
    """the carried arrays of an engine (host copies, uint32; cold / infectees as [n, 8]).  Stays beside reports.host_state on
    purpose: the clone is checked on every buffer a day carries, read here by name with nothing of the package in between."""
    n = engine.config.n_agents
    out = {}
    for name in ('hot', 'cold', 'infectees', 'counters', 'control', 'queue0', 'queue1', 'level1', 'active_bits', 'infected_bits'):
        t = engine.tensors[name]
        a = np.array(t.cpu().numpy() if hasattr(t, 'cpu') else t).view(np.uint32)
        out[name] = a.reshape(n, -1) if name in ('cold', 'infectees') else a
    return out


def assert_same_day_state(a, b, planes=True):
    """two Contexts' carried state between days: hot words, counters, the cold records' infector, n_infected, onset and
    vacc_day, the infectee lists as sets of pairs (inline slots and overflow lists), the queues as multisets, both bit planes
    (unless planes=False: oracle B does not keep them).  (Claims are per-day: a restore resets them.)"""
    from shard_util import list_pairs
    x, y = carried(a.engine), carried(b.engine)
    for name in ('hot', 'counters') + (('active_bits', 'infected_bits') if planes else ()):
        bad = np.flatnonzero(x[name] != y[name])
        assert len(bad) == 0, '%s: %d words differ, first %d' % (name, len(bad), bad[0])
    bad = np.flatnonzero((x['cold'][:, 2:6] != y['cold'][:, 2:6]).any(axis=1))
    assert len(bad) == 0, 'cold: %d records differ, first %d' % (len(bad), bad[0])
    assert np.array_equal(list_pairs(a), list_pairs(b)), 'infectee lists'
    for k, q in enumerate(('queue0', 'queue1', 'level1')):
        ln = int(x['control'][filtering.L_QUEUE0 + k])
        assert ln == int(y['control'][filtering.L_QUEUE0 + k]), q
        assert np.array_equal(np.sort(x[q][:ln]), np.sort(y[q][:ln])), q


def continuation(v, ages, seeds, a, m, cut, days, engine_factory=None, device='cuda:0'):
    """Run a group of `seeds` for `cut` days, clone member a into member m, run `days` more as a group.  Returns (member m's
    history of the last `days` days, its Context, the history and Context of a restore of a snapshot of seeds[a]'s run at
    `cut` into a fresh Context with seed seeds[m], run `days` days alone)."""
    setup = ensemble.Setup(ages, device, engine_factory, None, 'auto')
    planner, ctxs = setup.planner(v, seeds[0]), setup.members(v, seeds)
    group, _ = ensemble.group_for(ctxs)
    try:
        ensemble.run_group_plan(ctxs, planner.make_plan(cut), group=group)
        filtering.clone_group(group, [(m, a)])
        hist = ensemble.run_group_plan(ctxs, planner.make_plan(days), group=group)
    finally:
        group.close()
    solo = setup.context(v, seeds[a])
    solo.run(cut)
    snap = solo.snapshot()
    ref = simulation.make_context(v, age_counts=ages, seed=seeds[m], device=device, engine_factory=engine_factory, snapshot=snap)
    return hist[m], ctxs[m], ref.run(days), ref
