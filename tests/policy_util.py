"""Test-side definitions of the policy tests (reina_model_amd/policy.py): the scenarios, policies and thresholds the CPU and
the GPU tests share, in ONE place.  tests/test_policy.py asserts on oracle B that these inputs exercise what the GPU tests
need (escalations, a relaxation, members that switch on different days); tests/test_policy_gpu.py runs them on the device."""
import copy

import numpy as np

from reina_model_amd import engine as eng
from reina_model_amd import policy as pol
from reina_model_amd import simulation
from reina_model_amd.variables import VARIABLE_DEFAULTS

HUS_DAYS = 365
GROUP_SEEDS = list(range(100, 132))   # the 32 seeds of the group tests
GROUP_HUS_DAYS = 120
MINI_AGENTS = 20000
MINI_DAYS = 200
BRANCH_DAY = 120                       # the snapshot the branches fork from
BRANCH_DAYS = 60
BRANCH_SEEDS = [7, 8, 9, 10]


def hus_variables():
    return copy.deepcopy(VARIABLE_DEFAULTS)


def mini_scenario():
    from filter_util import small_scenario
    return small_scenario(MINI_AGENTS)


def ward_policy():
    """the HUS policy: people in ward, reviewed weekly, three levels"""
    return pol.Policy(pol.Signal('in_ward'),
                      levels=[[], [['limit-mobility', 30]], [['limit-mobility', 50], ['wear-masks', 40]]],
                      up=[200, 600], down=[100, 400], review_every=7, min_days=14)


def mini_policy():
    """the mini population's: detected cases of the last 7 days, reviewed daily"""
    return pol.Policy(pol.Signal('all_detected', 'increment', 7),
                      levels=[[], [['limit-mobility', 40]], [['limit-mobility', 60], ['wear-masks', 50, None, None, 'work']]],
                      up=[MINI_UP[0], MINI_UP[1]], down=[MINI_DOWN[0], MINI_DOWN[1]], review_every=1, min_days=5)


MINI_UP = (750, 820)
MINI_DOWN = (400, 600)


def rows_policy():
    """levels whose row structure differs: level 1 an age-windowed limit-mobility (it splits classes of the contact matrix, so
    the tables hold more distinct rows), level 2 a place-only one"""
    return pol.Policy(pol.Signal('in_ward'),
                      levels=[[], [['limit-mobility', 35, 23, 67]], [['limit-mobility', 55, None, None, 'leisure']]],
                      up=[200, 600], down=[100, 400], review_every=5, min_days=7)


def masks_policy():
    """a level made of wear-masks alone"""
    return pol.Policy(pol.Signal('in_ward'), levels=[[], [['wear-masks', 60]]], up=[200], down=[80], review_every=7, min_days=14)


def never_policy():
    return pol.Policy(pol.Signal('dead'), levels=[[], [['limit-mobility', 30]]], up=[2 ** 31 - 1], down=[0])


def forced_policy(start):
    """level 1 = limit-mobility 30 from `start` (an ISO date) on: threshold 0 is always met"""
    return pol.Policy(pol.Signal('infected'), levels=[[], [['limit-mobility', 30]]], up=[0], down=[0], start=start)


def make(v, ages=None, seed=1, factory=None, policy=None, device='cuda:0', ipc='auto', interventions=None, snapshot=None):
    return simulation.make_context(v, age_counts=ages, seed=seed, device=device, engine_factory=factory, ipc=ipc, policy=policy,
                                   interventions=interventions, snapshot=snapshot)


def switches(levels):
    """(days of escalation, days of relaxation) of a level trace"""
    lv = np.asarray(levels, dtype=np.int64)
    prev = np.concatenate([[0], lv[:-1]])
    return np.flatnonzero(lv > prev), np.flatnonzero(lv < prev)


def first_escalation(levels):
    up, _ = switches(levels)
    return int(up[0]) if len(up) else -1


def hot_cold(ctx):
    """(hot words, cold records' infector / n_infected / onset / vacc_day) of a Context's engine, host copies"""
    n = ctx.engine.config.n_agents
    out = []
    for name in ('hot', 'cold'):
        t = ctx.engine.tensors[name]
        a = np.array(t.cpu().numpy() if hasattr(t, 'cpu') else t).view(np.uint32)
        out.append(a if name == 'hot' else a.reshape(n, eng.COLD_WORDS)[:, 2:6])
    return out


def assert_same_run(a, b, hist_a, hist_b, planes):
    """two policy runs: history, levels, mobility factors and the final state -- between two engines of one kind everything a
    day carries over (bit planes included), against oracle B (planes=False) the hot words, the counters and the cold records:
    oracle B keeps no bit planes, and the two keep the contact-tracing work list of a finished day differently"""
    from filter_util import assert_same_day_state
    bad = np.argwhere(np.asarray(hist_a) != np.asarray(hist_b))
    assert len(bad) == 0, 'history: %d words differ, first at (day, word) %s' % (len(bad), bad[0])
    assert np.array_equal(a.policy_levels, b.policy_levels), 'levels'
    assert list(a.mobility_history) == list(b.mobility_history), 'mobility factors'
    if planes:
        assert_same_day_state(a, b, planes=True)
        return
    for name, x, y in zip(('hot', 'cold'), hot_cold(a), hot_cold(b)):
        bad = np.flatnonzero((x != y).reshape(len(x), -1).any(axis=1))
        assert len(bad) == 0, '%s: %d agents differ, first %d' % (name, len(bad), bad[0])
    assert np.array_equal(a.engine.read_counters(), b.engine.read_counters()), 'counters'
