"""Test-side definitions of the policy tests (reina_model_amd/policy.py): the scenarios, policies and thresholds the CPU and
the GPU tests share, in ONE place.  tests/test_policy.py asserts on oracle B that these inputs exercise what the GPU tests
need (escalations, a relaxation, members that switch on different days); tests/test_policy_gpu.py runs them on the device."""
import collections
import copy
import zlib
from datetime import date, timedelta

import numpy as np

from reina_model_amd import engine as eng
from reina_model_amd import policy as pol
from reina_model_amd import simulation
from reina_model_amd.dayrun import History
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
    """(hot words, cold records' infector / n_infected / onset / vacc_day) of a Context's engine, host copies.  Stays beside
    reports.host_state on purpose: that one hands out two of the four cold fields, and this compares whole runs by all four."""
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


# ------------------------------------------------------------------------------------------------ the rule on driven signals
#
# k_policy fed with signals written into a counter row, not with what an epidemic happens to produce.  An idle population (no
# initial condition, no interventions) keeps a written row as it is through its days; a live run of mini_scenario(), which
# has no vaccination programme, keeps the `vaccinated` row.  tests/test_policy.py asserts both on oracle B and that the inputs
# below take every branch of the rule; tests/test_policy_rule_gpu.py runs them on the device.

START_DATE = VARIABLE_DEFAULTS['start_date']
RULE_MEMBERS = 6
WORD_BAND = 4000000        # |word| of the 127 free words of a row: the sum of all 128 absolute values stays below 2 ** 31
VALUE_BOUND = 7000000      # |x_now| the generators stay within

Rule = collections.namedtuple('Rule', 'kind n_days up down review_every min_days start_day')
BRANCHES = ('step', 'jump', 'rise_at_up', 'stay_at_down', 'relax', 'held', 'no_review_rise', 'clipped', 'full', 'gap', 'negative')


def rule_of(policy, start_date=START_DATE):
    return Rule(policy.signal.kind, policy.signal.days, tuple(policy.up), tuple(policy.down), policy.review_every,
                policy.min_days, policy.start_day(start_date))


def walk_rule(days, x_now, rule):
    """The rule of include/reina_policy.h over the whole list of days seen (ascending day numbers, their x_now): every value
    is kept under its day, x(d) = x_now(d) - x_now(max(d - n, first)) is looked up, `first` restarts when a day does not
    follow the last one seen.  Returns ([(level in force, x)] per day, a Counter of the branches taken: BRANCHES, and
    'window_at_first' for the days whose d - n is exactly `first`)."""
    L = len(rule.up) + 1
    seen, out, took = {}, [], collections.Counter()
    level, governed, first, last = 0, 0, None, None
    for d, v in zip(days, x_now):
        d, v = int(d), int(v)
        if last is None or d != last + 1:
            took['gap'] += last is not None
            first = d
        seen[d] = v
        x = v
        if rule.kind == 'increment':
            took['clipped' if d - rule.n_days < first else 'full'] += 1
            took['window_at_first'] += d - rule.n_days == first
            x = v - seen[max(d - rule.n_days, first)]
        took['negative'] += x < 0
        reach = max([j for j in range(level + 1, L) if x >= rule.up[j - 1]], default=level)
        if d >= rule.start_day and (d - rule.start_day) % rule.review_every == 0:
            if reach > level:
                took['jump' if reach - level >= 2 else 'step'] += 1
                took['rise_at_up'] += x == rule.up[reach - 1]
                level, governed = reach, 0
            elif level > 0:
                took['stay_at_down'] += x == rule.down[level - 1]
                if x < rule.down[level - 1]:
                    if governed >= rule.min_days:
                        took['relax'] += 1
                        level, governed = level - 1, 0
                    else:
                        took['held'] += 1
        else:
            took['no_review_rise'] += reach > level
        governed += 1
        last = d
        out.append((level, x))
    return out, took


def spread(value, rng):
    """int32[MAX_AGES] of mixed signs that sum to `value`, the ages at and above nr_ages included; the sum of the absolute
    values stays below 2 ** 31, so every summation order in int32 gives `value`"""
    assert abs(int(value)) <= VALUE_BOUND
    w = rng.integers(-WORD_BAND, WORD_BAND + 1, size=eng.MAX_AGES).astype(np.int64)
    k = int(rng.integers(0, eng.MAX_AGES))
    w[k] = 0
    w[k] = int(value) - int(w.sum())
    assert int(np.abs(w).sum()) < 2 ** 31 and int(w.sum()) == int(value)
    return w.astype(np.int32)


def signal_range(policy):
    r = policy.signal.row * eng.MAX_AGES
    return r, r + eng.MAX_AGES


def ladder(n_levels, step=10):
    """n_levels levels of one row structure: population-wide mobility limits"""
    return [[]] + [[['limit-mobility', step * j]] for j in range(1, n_levels)]


class DrivenCase:
    """One policy and what drives it: `calls` [(first day, days, seen)] cover the days [0, total) in order -- seen: a run_days
    call of the policy, not seen: days handed to the plain sink (the days before the first one seen, the gaps); `days`: the
    days seen; `values[m][i]`: member m's x_now on days[i], constant within a call (the row is written before the call)."""

    def __init__(self, name, policy, calls, values, agents=700, seeds=None, live=False):
        self.name, self.policy, self.calls, self.agents, self.live = name, policy, list(calls), agents, live
        self.rule = rule_of(policy)
        self.total = sum(n for _, n, _ in self.calls)
        self.days = [d for a, n, seen in self.calls if seen for d in range(a, a + n)]
        self.values = [list(v) for v in values]
        self.members = len(self.values)
        self.seeds = list(seeds) if seeds is not None else list(range(1, self.members + 1))
        assert all(len(v) == len(self.days) for v in self.values)
        at = {d: i for i, d in enumerate(self.days)}
        rng = np.random.default_rng(hash_name(name))
        self.call_value = [[v[at[a]] if seen else None for a, n, seen in self.calls] for v in self.values]
        for m, v in enumerate(self.values):
            for a, n, seen in self.calls:
                assert not seen or len(set(v[at[a]:at[a] + n])) == 1
        self.rows = [[None if x is None else spread(x, rng) for x in cv] for cv in self.call_value]
        self.walked = [walk_rule(self.days, v, self.rule) for v in self.values]

    def levels(self, m):
        return np.array([lv for lv, _ in self.walked[m][0]], dtype=np.int32)

    def trace(self, m):
        """[total, 2]: the walker's (level, x) on the days seen, 0 on the others"""
        t = np.zeros((self.total, pol.TRACE_WORDS), dtype=np.int32)
        t[self.days] = np.array(self.walked[m][0], dtype=np.int64).astype(np.int32)
        return t

    def written(self, m):
        """[total, MAX_AGES]: what history row d must hold in the signal row -- the last row written, 0 before the first"""
        out = np.zeros((self.total, eng.MAX_AGES), dtype=np.int32)
        cur = out[0].copy()
        for (a, n, seen), row in zip(self.calls, self.rows[m]):
            if row is not None:
                cur = row
            out[a:a + n] = cur
        return out

    def one(self, m):
        """member m alone, with the rows it has here"""
        c = copy.copy(self)
        c.name, c.members = '%s/%d' % (self.name, m), 1
        for attr in ('values', 'seeds', 'call_value', 'rows', 'walked'):
            setattr(c, attr, [getattr(self, attr)[m]])
        return c


def hash_name(name):
    """a seed from a case's name, the same in every process"""
    return zlib.crc32(name.encode())


def _cut(rng, n):
    """n days cut into calls of 1..5"""
    out = []
    while n:
        k = min(n, int(rng.choice([1, 2, 3, 4, 5], p=[.4, .2, .15, .1, .15])))
        out.append(k)
        n -= k
    return out


def _calls(rng, start, gaps, runs):
    calls, d = [], 0
    if start:
        calls.append((0, start, False))
        d = start
    for i, ln in enumerate(runs):
        for k in _cut(rng, ln):
            calls.append((d, k, True))
            d += k
        if i < len(gaps):
            calls.append((d, gaps[i], False))
            d += gaps[i]
    return calls


def _level_values(rng, rule, calls, never):
    thr = sorted(set(rule.up + rule.down))
    lo, hi = thr[0], thr[-1]
    span = max(hi - lo, 8)
    out = []
    for a, n, seen in calls:
        if not seen:
            continue
        u = rng.random()
        if never:
            v = rule.up[0] - 1 - int(rng.integers(0, span))
        elif u < .45:
            v = int(rng.choice(thr)) + int(rng.integers(-1, 2))
        elif u < .7:
            v = lo - 1 - int(rng.integers(0, span // 4 + 1))
        else:
            v = int(rng.integers(lo - span // 4, hi + span // 4 + 1))
        out += [v] * n
    return out


def _increment_values(rng, rule, calls, never):
    """a walk whose steps are comparable to the thresholds; where the window allows, a call's value is set so that x lands on
    a threshold or beside it"""
    assert rule.up[0] > 0
    thr = sorted(set(rule.up + rule.down))
    step = max(2, int(rule.up[-1] / max(1.0, rule.n_days / 2.5) ** .5))
    seen, out, prev, first, last = {}, [], 0, None, None
    for a, n, is_seen in calls:
        if not is_seen:
            continue
        if last is None or a != last + 1:
            first = a
        back = max(a - rule.n_days, first)
        if never:
            v = prev - int(rng.integers(0, step + 1))
        elif back != a and rng.random() < .45:
            v = seen[back] + int(rng.choice(thr)) + int(rng.integers(-1, 2))
        else:
            v = prev + int(rng.integers(-step, 2 * step + 1))
        for d in range(a, a + n):
            seen[d] = v
        out += [v] * n
        prev, last = v, a + n - 1
    return out


def _rule_case(name, signal, n_levels, up, down, review_every, min_days, start_day, first_day, gaps, runs, agents):
    start = None if start_day == 0 else (date.fromisoformat(START_DATE) + timedelta(days=start_day)).isoformat()
    policy = pol.Policy(signal, ladder(n_levels), up=up, down=down, review_every=review_every, min_days=min_days, start=start)
    rule = rule_of(policy)
    rng = np.random.default_rng(hash_name(name) + RULE_SEED)
    calls = _calls(rng, first_day, gaps, runs)
    gen = _level_values if rule.kind == 'level' else _increment_values
    values = [gen(rng, rule, calls, never=m == RULE_MEMBERS - 1) for m in range(RULE_MEMBERS)]
    return DrivenCase(name, policy, calls, values, agents=agents)


RULE_SEED = 1
_S = pol.Signal
# name, signal, L, up, down, review_every, min_days, start_day, first day seen, gaps, unbroken runs, agents
RULE_CASES = [_rule_case(*c) for c in (
    ('eight-level-equal-ups', _S('in_ward'), 8, [10, 20, 20, 40, 50, 60, 70], [5, 20, 12, 30, 45, 55, 65], 1, 0, 0, 0, (1, 40), (20, 68, 14), 700),
    ('eight-increment-7', _S('vaccinated', 'increment', 7), 8, [100, 200, 300, 400, 400, 600, 700], [50, 150, 300, 350, 380, 500, 650], 3, 2, 4, 3, (5, 1), (70, 12, 20), 2000),
    ('five-increment-28', _S('in_ward', 'increment', 28), 5, [1000, 2000, 3000, 5000], [-500, 1000, 2500, 4000], 1, 9, 0, 30, (40, 5), (14, 68, 20), 300),
    ('five-negative', _S('in_ward'), 5, [-300, -200, -100, 0], [-350, -250, -100, -50], 7, 0, 11, 3, (1, 5), (36, 30, 36), 1100),
    ('three-increment-1', _S('vaccinated', 'increment', 1), 3, [5, 50], [-5, 5], 1, 2, 0, 0, (40, 1), (66, 16, 20), 513),
    ('three-increment-27', _S('in_ward', 'increment', 27), 3, [20000, 50000], [0, 30000], 3, 0, 11, 30, (5, 40), (30, 70, 6), 1500),
    ('two-weekly', _S('in_ward'), 2, [1000000], [999000], 7, 9, 4, 3, (1, 1), (40, 34, 28), 450),
    ('two-increment-down-is-up', _S('vaccinated', 'increment', 7), 2, [60], [60], 1, 0, 0, 0, (5, 40), (68, 22, 12), 900),
    ('eight-level-every-3', _S('vaccinated'), 8, [-40, 0, 1000, 1001, 50000, 50000, 3000000], [-41, -20, 500, 1001, 2000, 50000, 1000000], 3, 2, 11, 30, (1, 5), (24, 66, 12), 2000),
    ('eight-level-daily-held', _S('in_ward'), 8, [3, 6, 9, 12, 15, 18, 21], [1, 4, 7, 10, 13, 16, 19], 1, 2, 4, 3, (40, 5), (66, 20, 16), 1024),
)]
SINGLE_RULE_CASES = ('eight-increment-7', 'eight-level-equal-ups')   # run for one engine too (k_policy<false>)


def _switch_case():
    """the live epidemic's: eight levels of differing row structure on mini_scenario(), driven through its `vaccinated` row"""
    levels = [[], [['limit-mobility', 35, 23, 67]], [['limit-mobility', 55, None, None, 'leisure']], [['wear-masks', 60]],
              [['wear-masks', 60]], [['limit-mobility', 40]], [['limit-mobility', 50, 10, 40], ['wear-masks', 40, None, None, 'work']],
              [['limit-mobility', 70], ['wear-masks', 50]]]
    up, down = list(range(10, 80, 10)), list(range(5, 75, 10))
    policy = pol.Policy(pol.Signal('vaccinated'), levels, up=up, down=down, review_every=1, min_days=0)
    sched = [(6, 0)]
    for j in range(1, 8):                       # every jump 0 -> j, and back one level a day: the last chain is 7 -> 0
        sched += [(1, up[j - 1] + j % 2)] + [(1, -3)] * min(j, 2) + ([(j - 2, -3 - j)] if j > 2 else [])
    sched += [(1, 10), (1, 20), (1, 35), (1, 48), (20, 47), (1, 72), (15, 66), (3, 0), (10, 40), (1, 22), (7, 30),
              (1, 61), (1, 25), (10, 50), (30, 12), (16, 71)]      # (1, 61) is day 102, the scenario's dated table change
    calls, vals, d = [], [], 0
    for n, v in sched:
        calls.append((d, n, True))
        vals += [v] * n
        d += n
    # three more members for the group run: the same calls, other values
    members = [vals]
    per_call = [v for _, v in sched]
    for m in (1, 2, 3):
        shifted = per_call[7 * m:] + per_call[:7 * m]
        members.append([v + m for (n, _), v in zip(sched, shifted) for _ in range(n)])
    return DrivenCase('switch', policy, calls, members, agents=MINI_AGENTS, seeds=[1, 2, 3, 4], live=True)


SWITCH_DATED_DAY = 102
SWITCH_CASE = _switch_case()


def make_driven(case, m=0, factory=None, policy=None):
    """member m's Context of a driven case: idle (no initial condition, no interventions) or the live mini scenario"""
    if case.live:
        v, ages = mini_scenario()
        return make(v, ages, seed=case.seeds[m], factory=factory, policy=policy)
    from snap_util import population
    return make(hus_variables(), population(case.agents), seed=case.seeds[m], factory=factory, policy=policy, ipc=None, interventions=[])


def write_row(ctx, policy, words):
    """a signal row into a Context's counter block.  On the device the copy is queued on torch's current stream, which is
    the stream the library's launches are queued on (engine.alloc.stream()), as tx_util.put_forest's callers rely on."""
    a, b = signal_range(policy)
    t = ctx.engine.tensors['counters']
    if hasattr(t, 'copy_'):
        import torch
        t[a:b].copy_(torch.from_numpy(np.ascontiguousarray(words, dtype=np.int32)))
    else:
        np.asarray(t)[a:b] = words
    eng.mark_stale([ctx.engine])


def run_driven_context(ctx, case, m=0, policy_on_context=False):
    """Member m of `case` on one Context, call by call, the row written before each: the calls seen by Context.run with the
    policy attached (policy_on_context: the device route) or by policy.run_host_driven, the others by a plain Context.run.
    Returns the history [total, COUNTER_WORDS]; ctx.policy_levels / ctx.mobility_history cover the days seen."""
    hist, levels, mobility = [], [], []
    policy = case.policy
    if policy_on_context:
        assert ctx.policy is policy
    for (a, n, seen), row in zip(case.calls, case.rows[m]):
        assert ctx.day == a
        if seen:
            write_row(ctx, policy, row)
            hist.append(ctx.run(n) if policy_on_context else pol.run_host_driven(ctx, policy, n))
            levels.append(np.asarray(ctx.policy_levels))
            mobility += list(ctx.mobility_history)
        else:
            keep, ctx.policy = ctx.policy, None
            hist.append(ctx.run(n))
            ctx.policy = keep
    ctx.policy_levels = np.concatenate(levels).astype(np.int32)
    ctx.mobility_history = mobility
    return np.concatenate(hist)


class DrivenDeviceRun:
    """`case` on the device through ONE DevicePolicy for an engine group of its members (or for one engine: a case of one
    member, group=False): the day descriptors of a planner's make_plan, every member's row written before each call seen,
    the other days handed to the plain sink (after a read_trace that ends on the last day run, as include/reina_policy.h
    asks of a caller that goes on without the policy).  The bank is uploaded at the start of every stretch of dated tables
    -- once for an idle population.  Keeps: ctxs, dev, history [members, total, COUNTER_WORDS], trace [members, total, 2]."""

    def __init__(self, case, group=True, before_call=None):
        self.case = case
        policy = case.policy
        self.ctxs = ctxs = [make_driven(case, m) for m in range(case.members)]
        assert group or case.members == 1
        plan = make_driven(case).make_plan(case.total, policy=policy)
        day_list, seg_start = [], {}
        for si, (tables, arr, n) in enumerate(plan['segments']):
            seg_start[len(day_list)] = (si, tables)
            day_list += [arr[k] for k in range(n)]
        assert [d.day for d in day_list] == list(range(case.total))
        if group:
            self.group = eng.EngineGroup([c.engine for c in ctxs])
            self.dev = dev = pol.DevicePolicy(policy, START_DATE, group=self.group)
            plain, hist = self.group, History(case.total, True, group=self.group)
        else:
            self.group = None
            self.dev = dev = pol.DevicePolicy(policy, START_DATE, engine=ctxs[0].engine)
            plain, hist = ctxs[0].engine, History(case.total, True, ctx=ctxs[0])
        self.plan, self.day_list = plan, day_list
        bank, tables, policy_ran = None, None, False
        for ci, (a, n, seen) in enumerate(case.calls):
            if seen:
                for m, c in enumerate(ctxs):
                    write_row(c, policy, case.rows[m][ci])
            elif policy_ran:
                dev.read_trace(a - 1, 1)        # the members' host-side table mirrors follow their levels
                policy_ran = False
            cuts = sorted({a, a + n} | {s for s in seg_start if a < s < a + n})
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                if lo in seg_start:
                    bank, tables = seg_start[lo]
                if seen and bank is not None:
                    dev.upload_bank(plan['policy_banks'][bank][0])
                    bank = tables = None
                elif not seen and tables is not None:
                    plain.upload_contact_tables(*tables)
                    tables = None
                if before_call is not None:
                    before_call(self, lo, hi, seen)
                (dev if seen else plain).run_day_array((eng.Day * (hi - lo))(*day_list[lo:hi]), hi - lo, hist.at(lo))
                policy_ran = policy_ran or seen
        self.trace = dev.read_trace(0, case.total)
        seg_of_day, factors = pol.plan_segments_of_days(plan), [b[1] for b in plan['policy_banks']]
        for m, c in enumerate(ctxs):
            c._replayed = True
            pol._end_device_run(c, self.trace, m, 0, plan['mobility_history'][0], seg_of_day, factors)
            c.day = case.total
        h = hist.to_host()
        self.history = h if group else np.asarray(h)[None]
        if group:
            for c in ctxs:
                c._raise_on_problem(c.engine.read_counters())

    def close(self):
        self.dev.close()
        if self.group is not None:
            self.group.close()
