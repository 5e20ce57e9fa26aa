"""Triggered interventions (reina_model_amd/policy.py) on the CPU: the rule against hand-written sequences, the plain
formulation (run_host_driven) on oracle B against dated runs, the level tables against the dated uploads, and the conditions
the GPU tests' inputs must meet (tests/policy_util.py holds them)."""
import collections
import copy

import numpy as np
import pytest

from reina_model_amd import engine as eng
from reina_model_amd import ensemble, policy as pol
from par_backend import par_engine_factory
import policy_util as pu


def _row(p, value):
    c = np.zeros(eng.COUNTER_WORDS, dtype=np.int32)
    r = p.signal.row * eng.MAX_AGES
    c[r + 3] = value // 2
    c[r + 90] = value - value // 2
    return c


def _trace(p, values, first_day=0, start_day=0):
    st = p.new_state(start_day=start_day)
    return [pol.step_numpy(st, _row(p, v), first_day + k) for k, v in enumerate(values)]


def _policy(kind='level', days=7, levels=3, **kw):
    lv = [[], [['limit-mobility', 30]], [['limit-mobility', 50]], [['limit-mobility', 70]]][:levels]
    return pol.Policy(pol.Signal('in_ward', kind, days), lv, **kw)


# ---------------------------------------------------------------------------------------------- 1. the rule

def test_step_escalation_by_a_jump_and_at_equality():
    p = _policy(up=[10, 20], down=[5, 15])
    assert _trace(p, [9, 10, 19, 20]) == [0, 1, 1, 2]          # x == up[j - 1] escalates
    assert _trace(p, [0, 25, 25]) == [0, 2, 2]                 # 0 -> 2 in one step
    assert _trace(p, [0, 20]) == [0, 2]


def test_step_relaxes_one_level_at_a_time_and_not_at_equality():
    p = _policy(up=[10, 20], down=[5, 15])
    assert _trace(p, [25, 0, 0, 0]) == [2, 1, 0, 0]
    assert _trace(p, [25, 15, 14, 5, 4]) == [2, 2, 1, 1, 0]    # x == down[l - 1] holds the level


def test_step_min_days_holds_a_level():
    p = _policy(up=[10, 20], down=[5, 15], min_days=3)
    # level 2 decided on day 0 has governed 1, 2, 3 days before days 1, 2, 3
    assert _trace(p, [25, 0, 0, 0, 0, 0, 0, 0]) == [2, 2, 2, 1, 1, 1, 0, 0]
    # escalation does not wait
    assert _trace(p, [12, 25]) == [1, 2]


def test_step_review_cadence_and_start():
    p = _policy(up=[10, 20], down=[5, 15], review_every=3)
    assert _trace(p, [12, 25, 25, 25, 0, 0, 0], start_day=0) == [1, 1, 1, 2, 2, 2, 1]
    assert _trace(p, [12, 12, 12, 12, 12, 12], start_day=4) == [0, 0, 0, 0, 1, 1]
    # the cadence hangs on the calendar, not on the first day seen
    assert _trace(p, [12, 12, 12, 12], first_day=10, start_day=0) == [0, 0, 1, 1]


def test_step_increments_before_the_ring_is_full():
    p = _policy('increment', 3, levels=2, up=[6], down=[2])
    # x(d) = x_now(d) - x_now(max(d - 3, first)); first = 5
    vals = [100, 102, 104, 106, 108, 109, 109, 109, 109]
    st = p.new_state()
    xs = []
    for k, v in enumerate(vals):
        pol.step_numpy(st, _row(p, v), 5 + k)
        xs.append(st['x'])
    assert xs == [0, 2, 4, 6, 6, 5, 3, 1, 0]
    assert _trace(p, vals, first_day=5) == [0, 0, 0, 1, 1, 1, 1, 0, 0]
    # a day that does not follow the last one seen starts a new sequence
    lvl = pol.step_numpy(st, _row(p, 500), 40)
    assert st['x'] == 0 and st['first_day'] == 40 and lvl == 0
    # the ring holds 32 days: an increment over 28 days across its wrap
    q = _policy('increment', 28, levels=2, up=[10 ** 6], down=[0])
    st = q.new_state()
    for d in range(100):
        pol.step_numpy(st, _row(q, d * d), d)
        assert st['x'] == d * d - max(d - 28, 0) ** 2


def test_signal_sums_all_ages_of_the_row():
    p = _policy(up=[10, 20], down=[5, 15])
    c = np.zeros(eng.COUNTER_WORDS, dtype=np.int32)
    r = p.signal.row * eng.MAX_AGES
    c[r:r + eng.MAX_AGES] = 1
    c[r - 1] = 1000
    c[r + eng.MAX_AGES] = 1000
    st = p.new_state()
    pol.step_numpy(st, c, 0)
    assert st['x'] == eng.MAX_AGES


# ---------------------------------------------------------------------------------------------- 2. never triggered == plain

def test_never_triggered_is_the_plain_run():
    v = pu.hus_variables()
    a, b = pu.make(v, factory=par_engine_factory), pu.make(v, factory=par_engine_factory)
    ha = pol.run_host_driven(a, pu.never_policy(), 200)
    hb = b.run(200)
    assert np.array_equal(ha, hb)
    assert not a.policy_levels.any() and len(a.policy_levels) == 200
    assert list(a.mobility_history) == list(b.mobility_history)
    for x, y in zip(pu.hot_cold(a), pu.hot_cold(b)):
        assert np.array_equal(x, y)
    from filter_util import assert_same_day_state
    assert_same_day_state(a, b, planes=False)
    # Context.run with the policy attached takes the same route on an engine without the policy entry points
    c = pu.make(v, factory=par_engine_factory, policy=pu.never_policy())
    assert c.engine.policy_f is None
    assert np.array_equal(c.run(200), hb) and not c.policy_levels.any()


def test_level0_tables_are_the_dated_uploads():
    v = pu.hus_variables()
    planner = pu.make(v, factory=par_engine_factory)
    matrix_before = copy.deepcopy(planner.contact_matrix.mobility_factors)
    plan = planner.make_plan(v['simulation_days'], policy=pu.ward_policy())
    plain = pu.make(v, factory=par_engine_factory).make_plan(v['simulation_days'])
    assert len(plan['segments']) == len(plan['policy_banks']) == len(plain['segments'])
    rebuilds = 0
    for (tables, arr, n), (t2, _, n2), (bank, factors) in zip(plan['segments'], plain['segments'], plan['policy_banks']):
        assert n == n2 and len(bank) == 3 and len(factors) == 3
        if tables is None:
            continue
        rebuilds += 1
        for x, y, z in zip(tables[:5], bank[0][:5], t2[:5]):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes() == np.asarray(z).tobytes()
        assert list(tables[5]) == list(bank[0][5])
        assert bank[1][0].tobytes() != tables[0].tobytes()      # level 1 limits mobility: other contact numbers
    # (the default scenario's 17 dated limit-mobility interventions fall on 11 dates: the tables are rebuilt once a day)
    assert rebuilds == 11 and sum(iv[0] == 'limit-mobility' for iv in v['interventions']) == 17
    assert plan['mobility_history'] == plain['mobility_history']
    assert matrix_before == []


def test_build_bank_leaves_the_planner_alone():
    v = pu.hus_variables()
    ctx = pu.make(v, factory=par_engine_factory)
    ctx.run(60)
    cm = ctx.contact_matrix
    before = (copy.deepcopy(cm.mobility_factors), cm.mask_probabilities.copy(), float(cm.mobility_factor), cm.tables,
              ctx._uploaded_mask.copy())
    bank, factors = pol.build_bank(ctx, pu.ward_policy())
    assert cm.mobility_factors == before[0] and np.array_equal(cm.mask_probabilities, before[1])
    assert float(cm.mobility_factor) == before[2] and cm.tables is before[3] and np.array_equal(ctx._uploaded_mask, before[4])
    assert factors[1] == float(np.float32(0.7)) and factors[2] == float(np.float32(0.5)) and factors[0] == before[2]
    # a level's mask shares are in its tables: level 2 wears masks
    assert np.array_equal(bank[0][4], before[4]) and not np.array_equal(bank[2][4], before[4])
    assert np.all(bank[2][4][:ctx.nr_ages, :6] == np.float32(0.4))


# ---------------------------------------------------------------------------------------------- 3. forced level == dated

def _windowed_interventions():
    """the default scenario without its population-wide mobility limits: every later dated change replaces the factor of a
    window that exists on FORCED_DATE"""
    return [iv for iv in pu.hus_variables()['interventions'] if not (iv[0] == 'limit-mobility' and len(iv) == 3)]


FORCED_DATE, FORCED_DAY = '2020-06-10', 113


def test_forced_level_is_the_dated_intervention():
    v, ages = pu.mini_scenario()
    ivs = _windowed_interventions()
    a = pu.make(v, ages, factory=par_engine_factory, interventions=ivs)
    b = pu.make(v, ages, factory=par_engine_factory, interventions=ivs + [['limit-mobility', FORCED_DATE, 30]])
    ha = pol.run_host_driven(a, pu.forced_policy(FORCED_DATE), 250)
    hb = b.run(250)
    assert list(a.policy_levels) == [0] * FORCED_DAY + [1] * (250 - FORCED_DAY)
    bad = np.argwhere(ha != hb)
    assert len(bad) == 0, 'first difference at (day, word) %s' % bad[0]
    # the reported factor is the one the LAST limit-mobility applied left: the level's own while it is in force (a later dated
    # change to another window, 2020-08-12 = day 176, takes the column over in the dated run)
    assert list(a.mobility_history[:177]) == list(b.mobility_history[:177])
    assert a.mobility_history[FORCED_DAY] != a.mobility_history[FORCED_DAY + 1] == float(np.float32(0.7))
    from filter_util import assert_same_day_state
    assert_same_day_state(a, b, planes=False)
    # ... and it is not the run without it
    c = pu.make(v, ages, factory=par_engine_factory, interventions=ivs)
    assert not np.array_equal(c.run(250), hb)


# ---------------------------------------------------------------------------------------------- 4. conditions on the GPU tests' inputs

def test_hus_policy_escalates_twice_and_relaxes():
    c = pu.make(pu.hus_variables(), factory=par_engine_factory)
    pol.run_host_driven(c, pu.ward_policy(), pu.HUS_DAYS)
    up, down = pu.switches(c.policy_levels)
    assert len(up) >= 2 and len(down) >= 1, (up, down)
    assert c.policy_levels.max() == 2
    # the other HUS policies of the GPU tests switch too
    for p in (pu.rows_policy(), pu.masks_policy()):
        c = pu.make(pu.hus_variables(), factory=par_engine_factory)
        pol.run_host_driven(c, p, pu.HUS_DAYS)
        up, down = pu.switches(c.policy_levels)
        assert len(up) >= 1 and len(down) >= 1 and set(c.policy_levels) == set(range(p.n_levels))


def test_group_seeds_switch_on_different_days():
    v, ages = pu.mini_scenario()
    hist, levels, ctxs = ensemble.run_policy_ensemble(v, pu.GROUP_SEEDS, pu.MINI_DAYS, pu.mini_policy(), age_counts=ages,
                                                      engine_factory=par_engine_factory)
    assert hist.shape == (32, pu.MINI_DAYS, eng.COUNTER_WORDS) and levels.shape == (32, pu.MINI_DAYS)
    firsts = [pu.first_escalation(lv) for lv in levels]
    assert len(set(f for f in firsts if f >= 0)) >= 3, firsts
    assert firsts.count(-1) >= 1, firsts
    assert levels.max() == 2


def test_row_structure_of_the_levels_differs():
    """the age-windowed level holds more distinct contact rows than the dated tables (the LDS carve of the GPU run)"""
    ctx = pu.make(pu.hus_variables(), factory=par_engine_factory)
    bank, _ = pol.build_bank(ctx, pu.rows_policy())
    rows = [len(np.unique(np.concatenate([np.asarray(t[2])[:ctx.nr_ages], np.asarray(t[0])[:ctx.nr_ages, None].view(np.uint32)], axis=1), axis=0))
            for t in bank]
    assert rows[1] > rows[0] and rows[2] == rows[0], rows


# ---------------------------------------------------------------------------------------------- 5. validation, refusals

@pytest.mark.parametrize('field, kw', [
    ('levels', dict(levels=[[]])),
    ('levels', dict(levels=[[]] * 9, up=[1] * 8, down=[0] * 8)),
    ('levels', dict(levels=[[], [['vaccinate', 1000]]])),
    ('up', dict(up=[30, 20], down=[5, 5], levels=[[], [], []])),
    ('up', dict(up=[1.5])),
    ('up', dict(up=[1, 2])),
    ('down', dict(down=[11])),
    ('down', dict(down=[])),
    ('review_every', dict(review_every=0)),
    ('min_days', dict(min_days=-1)),
    ('start', dict(start='10.6.2020')),
    ('signal', dict(signal='in_ward')),
])
def test_policy_validation_names_the_field(field, kw):
    args = dict(signal=pol.Signal('in_ward'), levels=[[], [['limit-mobility', 30]]], up=[10], down=[5])
    args.update(kw)
    with pytest.raises(ValueError, match='Policy.' + field):
        pol.Policy(**args)


def test_signal_validation():
    with pytest.raises(ValueError, match='Signal.counter'):
        pol.Signal('beds')
    with pytest.raises(ValueError, match='Signal.kind'):
        pol.Signal('in_ward', 'slope')
    for n in (0, 29):
        with pytest.raises(ValueError, match='Signal.days'):
            pol.Signal('in_ward', 'increment', n)
    for name in ('in_ward', 'in_icu', 'hospitalized', 'all_detected', 'dead', 'detected', 'infected'):
        assert eng.C_NAMES[pol.Signal(name).row] == name


def test_refusals():
    v, ages = pu.mini_scenario()
    p = pu.never_policy()
    with pytest.raises(ValueError, match='snapshot'):
        pu.make(v, ages, factory=par_engine_factory, policy=p).snapshot()
    sharded = pu.make(v, ages, factory=par_engine_factory, ipc=None)
    sharded.n_shards = 2
    with pytest.raises(ValueError, match='sharded'):
        pol.run_host_driven(sharded, p, 1)
    with pytest.raises(ValueError, match='sharded'):
        sharded.make_plan(1, policy=p)
    sharded.n_shards = 1
    with pytest.raises(ValueError, match='made with'):
        pu.make(v, ages, factory=par_engine_factory, policy=p).run_plan(pu.make(v, ages, factory=par_engine_factory).make_plan(3))
    with pytest.raises(ValueError, match='Policy.start'):
        pol.Policy(pol.Signal('dead'), [[], []], [1], [0], start='2019-01-01').start_day(v['start_date'])


def test_frames_carry_the_levels():
    from reina_model_amd import simulation
    v, ages = pu.mini_scenario()
    v['simulation_days'] = 80
    p = pol.Policy(pol.Signal('all_detected', 'increment', 7), [[], [['limit-mobility', 40]], [['limit-mobility', 60]]], up=[200, 10 ** 6],
                   down=[50, 100], review_every=2)
    df, adf = simulation.simulate_individuals(v, engine_factory=par_engine_factory, age_counts=ages, policy=p)
    plain, _ = simulation.simulate_individuals(v, engine_factory=par_engine_factory, age_counts=ages)
    assert 'policy_level' in df.columns and 'policy_level' not in plain.columns
    lv = df['policy_level'].to_numpy()
    assert lv.max() >= 1
    k = int(np.flatnonzero(lv > 0)[0])
    # the mobility column follows the level a day later (the state BEFORE a day)
    assert df['mobility_limitation'].iloc[k + 1] == pytest.approx(0.4)
    assert df['mobility_limitation'].iloc[k] == plain['mobility_limitation'].iloc[k]


# ---------------------------------------------------------------------------------------------- 7. the rule on driven signals

def _step_trace(case, m):
    """step_numpy over member m's days seen, fed the counter blocks the rows are written into: [(level, x)]"""
    st = case.policy.new_state(pu.START_DATE)
    lo, hi = pu.signal_range(case.policy)
    out = []
    for (a, n, seen), row in zip(case.calls, case.rows[m]):
        if not seen:
            continue
        c = np.zeros(eng.COUNTER_WORDS, dtype=np.int32)
        c[lo:hi] = row
        c[lo - 1] = c[hi % eng.COUNTER_WORDS] = 12345      # (the neighbouring rows are not the signal)
        for d in range(a, a + n):
            level = pol.step_numpy(st, c, d)
            out.append((level, st['x']))
    return out


@pytest.mark.parametrize('case', pu.RULE_CASES + [pu.SWITCH_CASE], ids=lambda c: c.name)
def test_walker_equals_step_numpy(case):
    for m in range(case.members):
        want, _ = case.walked[m]
        got = _step_trace(case, m)
        bad = [k for k in range(len(want)) if got[k] != want[k]]
        assert not bad, 'member %d, day %d: step_numpy %s, walker %s' % (m, case.days[bad[0]], got[bad[0]], want[bad[0]])


def _changes(case, m):
    """{day seen: the level in force differs from the one of the last day seen}"""
    lv = case.levels(m)
    return dict(zip(case.days, lv != np.concatenate([[0], lv[:-1]])))


def test_rule_cases_cover_what_the_issue_lists():
    rules = [c.rule for c in pu.RULE_CASES]
    assert len(rules) >= 8 and all(c.members == 6 and 95 <= len(c.days) <= 110 for c in pu.RULE_CASES)
    assert {len(r.up) + 1 for r in rules} == {2, 3, 5, 8} and {r.kind for r in rules} == {'level', 'increment'}
    assert {r.n_days for r in rules if r.kind == 'increment'} == {1, 7, 27, 28}
    assert {r.review_every for r in rules} == {1, 3, 7} and {r.min_days for r in rules} == {0, 2, 9}
    assert {r.start_day for r in rules} == {0, 4, 11}
    assert any(min(r.up) < 0 and min(r.down) < 0 for r in rules)
    assert any(r.up[j] == r.up[j + 1] for r in rules for j in range(len(r.up) - 1))
    assert any(r.down[j] == r.up[j] for r in rules for j in range(len(r.up)))
    firsts, gaps = set(), set()
    for c in pu.RULE_CASES:
        unseen = [n for _, n, seen in c.calls if not seen]
        firsts.add(c.days[0])
        gaps.update(unseen[1:] if c.days[0] else unseen)
        assert len(unseen) == 2 + (c.days[0] > 0) and all(1 <= n <= 5 for _, n, seen in c.calls if seen)
        # one member never crosses up[0]
        assert not c.levels(c.members - 1).any()
        # a row is 128 words of mixed sign, the ages at and above nr_ages among them, safe under any summation order
        for m in range(c.members):
            rows = np.array([r for r in c.rows[m] if r is not None], dtype=np.int64)
            assert (np.abs(rows).sum(axis=1) < 2 ** 31).all() and (rows < 0).any(axis=1).all() and (rows > 0).any(axis=1).all()
            assert (rows[:, 101:] != 0).any(axis=1).all()
            assert list(rows.sum(axis=1)) == [v for v in c.call_value[m] if v is not None]
    assert firsts == {0, 3, 30} and gaps == {1, 5, 40}


def test_rule_cases_take_every_branch():
    took = sum((c.walked[m][1] for c in pu.RULE_CASES for m in range(c.members)), start=collections.Counter())
    for b in pu.BRANCHES:
        assert took[b] >= 10, (b, took[b])
    assert took['window_at_first'] >= 1
    mid_call, first_day_change, quiet_call = 0, 0, 0
    for c in pu.RULE_CASES:
        eight = len(c.rule.up) == 7
        if eight:
            assert {int(x) for m in range(c.members) for x in c.levels(m)} == set(range(8)), c.name
        for m in range(c.members):
            ch = _changes(c, m)
            for a, n, seen in c.calls:
                if seen:
                    mid_call += sum(ch[d] for d in range(a + 1, a + n))
                    first_day_change += bool(ch[a])
                    quiet_call += not any(ch[d] for d in range(a, a + n))
        # the ring of an increment: a sequence that wraps it more than once, and one no longer than 20 days
        runs = np.split(np.array(c.days), np.flatnonzero(np.diff(c.days) != 1) + 1)
        assert c.rule.kind == 'level' or (max(len(r) for r in runs) > 2 * pol.RING and min(len(r) for r in runs) <= 20)
    assert mid_call >= 5 and first_day_change >= 1 and quiet_call >= 1


def test_switch_case_switches_where_the_issue_says():
    c = pu.SWITCH_CASE
    assert 150 <= c.total <= 200 and len(c.days) == c.total and c.rule.kind == 'level' and c.rule.review_every == 1
    assert c.policy.signal.counter == 'vaccinated' and c.policy.n_levels == 8 and c.rule.min_days == 0
    assert c.policy.levels[3] == c.policy.levels[4]
    assert not any(iv[0] == 'vaccinate' for iv in pu.mini_scenario()[0]['interventions'])
    lv = [int(x) for x in c.levels(0)]
    pairs = set(zip([0] + lv[:-1], lv))
    assert {(0, j) for j in range(1, 8)} <= pairs
    assert any(lv[k:k + 8] == [7, 6, 5, 4, 3, 2, 1, 0] for k in range(len(lv)))
    assert any(lv[k] < lv[k + 1] < lv[k + 2] for k in range(len(lv) - 2))       # escalations on consecutive days
    d = pu.SWITCH_DATED_DAY
    assert lv[d - 1] != lv[d] != lv[d + 1]
    # the levels' tables: an age window holds more distinct contact rows than the dated tables, a place-only limit and masks
    # alone hold as many; the two equal levels have the same bytes, every other neighbour differs
    ctx = pu.make_driven(c, 0, factory=par_engine_factory)
    bank, _ = pol.build_bank(ctx, c.policy)
    rows = [len(np.unique(np.concatenate([np.asarray(t[2])[:ctx.nr_ages], np.asarray(t[0])[:ctx.nr_ages, None].view(np.uint32)], axis=1), axis=0))
            for t in bank]
    assert rows[1] > rows[0] and rows[6] > rows[0] and rows[2] == rows[3] == rows[5] == rows[0], rows
    image = [b''.join(np.asarray(x).tobytes() for x in t[:5]) for t in bank]
    assert [image[k] == image[k + 1] for k in range(7)] == [False, False, False, True, False, False, False]
    # the members of the group run stand at different levels most days
    levels = np.stack([c.levels(m) for m in range(c.members)])
    assert (np.array([len(set(col)) for col in levels.T]) >= 3).mean() > .5


@pytest.mark.parametrize('case', pu.RULE_CASES, ids=lambda c: c.name)
def test_host_driver_on_an_idle_population(case):
    """the condition the GPU tests rest on: an idle population keeps a written row, and run_host_driven, fed the rows call by
    call, decides what the walker decides"""
    for m in range(case.members):
        ctx = pu.make_driven(case, m, factory=par_engine_factory)
        hist = pu.run_driven_context(ctx, case, m)
        lo, hi = pu.signal_range(case.policy)
        assert np.array_equal(hist[:, lo:hi], case.written(m)), 'member %d: the signal row did not stay as written' % m
        assert np.array_equal(ctx.policy_levels, case.levels(m)), 'member %d' % m


def test_host_driver_on_the_live_epidemic():
    case = pu.SWITCH_CASE
    ctx = pu.make_driven(case, 0, factory=par_engine_factory)
    hist = pu.run_driven_context(ctx, case, 0)
    lo, hi = pu.signal_range(case.policy)
    assert np.array_equal(hist[:, lo:hi], case.written(0)), 'the live run touched the vaccinated row'
    assert np.array_equal(ctx.policy_levels, case.levels(0))
    plain = pu.make_driven(case, 0, factory=par_engine_factory).run(case.total)
    ai = eng.C_NAMES.index('all_infected') * eng.MAX_AGES
    assert plain[-1, ai:ai + eng.MAX_AGES].sum() != hist[-1, ai:ai + eng.MAX_AGES].sum()
    assert np.array_equal(plain[:6], np.concatenate([hist[:6, :lo], plain[:6, lo:hi], hist[:6, hi:]], axis=1))   # (level 0 until day 6)
