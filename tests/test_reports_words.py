"""The words of every report, as they were before the reports' Python side got one shared core (reina_model_amd/reports.py):
the three numpy specifications on synthetic forests and on the states the shared pieces can get wrong, every route of a
60-day oracle-B run with a log, and the refusals.  Every case is the sha256 of the report's words, its scalars by name, or the
type and text of the exception it raised.

The expected results (tests/test_reports_words.json) were recorded with this very file on commit ff3913d, the last one on which
transmission.py, txlog.py and lineage.py each carried their own copy of those pieces: `python tests/test_reports_words.py
--record` rewrites the file from the code as it stands, which is only ever right on a commit whose words are the ones to keep."""
import functools
import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (HERE, os.path.dirname(HERE)) if p not in sys.path]   # (for `python tests/test_reports_words.py --record`)
import lineage_util as lu
import par_backend
import tx_util
import txlog_util as tu
from filter_util import small_scenario
from reina_model_amd import engine as eng
from reina_model_amd import ensemble, lineage as lin, simulation, transmission as tx, txlog as txl

WORDS = os.path.join(HERE, 'test_reports_words.json')
SIZES = (1, 511, 513, 3 * 512 + 7)
SHALLOW = 2                       # max_depth of the shallow cases: 2 rounds, chains of more than 3 links stay unconverged
PERIODS = (7, 43)
DAYS, AGENTS = 60, 20000

# The period checks of lineage.py are stated once since the shared core; the specification's route took the wording of the
# Context's (docs/HISTORY.md).  The type is the recorded one; these are the texts that replaced the recorded texts.
REWORDED = {'period_days must be in [1, 4096]': 'period must be in [1, 4096] days',
            'n_periods must be in [1, 256]': 'n_periods = {}: a lineage report holds 1 .. 256 periods (take a longer period)'}


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _result(fn):
    """what a call gave: a report (or a list of them) as hash and scalars, or the exception it raised"""
    try:
        r = fn()
    except Exception as e:        # noqa: BLE001  (the refusals are cases too)
        return dict(error=[type(e).__name__, str(e)])
    if isinstance(r, list):
        return [_result(lambda x=x: x) for x in r]
    if isinstance(r, str):
        return dict(sha256=r)
    module = {tx.TransmissionReport: tx, txl.LogReport: txl, lin.LineageReport: lin}[type(r)]
    return dict(words=_sha(r.words), scalars={name: int(getattr(r, name)) for name in module.SCALAR_NAMES},
                n_groups=int(r.n_groups), group_labels=r.group_labels)


def _three(hot, inf, cnt, log, age_start, groups, max_depth, n_days=tu.N_DAYS, periods=PERIODS):
    """one state through the three specifications"""
    return dict(tree=_result(lambda: tx.report_numpy(hot, inf, cnt, age_start, groups, max_depth)),
                log=_result(lambda: txl.report_numpy(hot, inf, cnt, log, age_start, groups, n_days)),
                lineage=_result(lambda: lin.report_numpy(hot, inf, cnt, log, age_start, groups, *periods, max_depth)))


def _forest(pattern, n, max_depth):
    hot, inf, cnt, log = tu.forest_state(n, pattern)
    return _three(hot, inf, cnt, log, tx_util.age_start_of(n), tx_util.groups('fine' if n % 2 else 'default'), max_depth)


def _state(n, agents, log=None):
    """(hot, infector, n_infected, log) of `agents`: (index, state, infector) triples; agent i's variant is i % 4, its
    infection day 3 * i, its onset two days later"""
    hot = np.zeros(n, dtype=np.uint32)
    inf = np.full(n, -1, dtype=np.int32)
    cnt = np.zeros(n, dtype=np.int32)
    words = np.full(n, txl.NONE << 16 | txl.NONE, dtype=np.uint32)
    for i, state, src in agents:
        hot[i], inf[i], words[i] = state | (i % 4) << 8 | 0x8000, src, (3 * i + 2) << 16 | 3 * i
        if 0 <= src < n:
            cnt[src] += 1
    return hot, inf, cnt, words


def _special(name, max_depth):
    n = 12
    age_start, groups = np.array([0, 4, 8, 12], dtype=np.int64), [0, 1, 2]
    chain = [(0, 5, -1), (1, 2, 0), (2, 1, 1), (3, 1, 2), (4, 1, 3), (5, 1, 4)]      # five links deep
    if name == 'none_infected':
        s = _state(n, [])
        s[1][[2, 5, 7]] = (5, 2, 40)                   # links among the susceptible: read by nobody
    elif name == 'self_link':
        s = _state(n, chain + [(8, 2, 8), (9, 1, 8)])
    elif name == 'infector_minus_2':
        s = _state(n, chain + [(8, 2, -2), (9, 1, 8)])
    elif name == 'infector_n':
        s = _state(n, chain + [(8, 2, n), (9, 1, 8)])
    elif name == 'link_to_state_0':
        s = _state(n, chain + [(8, 2, 7), (9, 1, 8)])
    elif name == 'cycle':
        s = lu.cycle_state()
        n, age_start = 10, np.array([0, 4, 8, 10], dtype=np.int64)
    elif name == 'combos':
        s = tu.combos_state()
        n = len(s[0])
        age_start, groups = tx_util.age_start_of(n), tx_util.groups()
    elif name == 'two_largest_trees':                  # trees of 3 under the roots 7 and 2, one of 2 under 0: the tie goes to 2
        s = _state(n, [(7, 5, -1), (8, 2, 7), (9, 1, 8), (2, 5, -1), (3, 1, 2), (11, 1, 2), (0, 1, -1), (1, 1, 0)])
    elif name == 'groups_up_to_15':
        n = 513
        s = tu.forest_state(n, 'random', seed=3)
        age_start, groups = tx_util.age_start_of(n), np.arange(tx_util.NR_AGES) % 16
    elif name == 'one_age':
        n = 513
        s = tu.forest_state(n, 'bad_links', seed=4)
        age_start, groups = np.array([0, n], dtype=np.int64), [3]
    else:
        raise KeyError(name)
    return _three(*s, age_start, groups, max_depth, n_days=tu.N_DAYS if name == 'combos' else 40)


SPECIAL = ('none_infected', 'self_link', 'infector_minus_2', 'infector_n', 'link_to_state_0', 'cycle', 'combos',
           'two_largest_trees', 'groups_up_to_15', 'one_age')


# ---------------------------------------------------------------------------------------------- a run on oracle B

def _oracle(seed, log=True):
    v, ages = small_scenario(AGENTS)
    c = simulation.make_context(v, age_counts=ages, seed=seed, ipc='auto', engine_factory=par_backend.par_engine_factory, txlog=log)
    c.run(DAYS)
    return c


@functools.lru_cache(maxsize=None)
def _runs():
    """two logged 60-day runs in host memory, and the first of them again without a log (a snapshot refuses one)"""
    return _oracle(3), _oracle(4), _oracle(3, log=False)


@functools.lru_cache(maxsize=None)
def _deep():
    """a Context of three days whose state is a chain of 300: deeper than its day + 1, so every report of it is taken twice"""
    v, ages = small_scenario(AGENTS)
    c = simulation.make_context(v, age_counts=ages, seed=9, ipc='auto', engine_factory=par_backend.par_engine_factory, txlog=True)
    n = c.engine.config.n_agents
    tx_util.put_forest(c, *tx_util.forest(n, 'chain', size=300), day=3)
    c.day = 3
    c.transmission_log.set_words(tu.random_log(n, top=3))
    return c


def _line_list(c):
    f = c.transmission_log.line_list()
    return _sha(np.stack([f[k].to_numpy().astype(np.int64) for k in f.columns])) + ' ' + ','.join(f.columns)


def _run(route):
    a, b, plain = _runs()
    log = a.transmission_log
    if route == 'snapshot':
        return _result(lambda: tx.report_from_snapshot(plain.snapshot(), plain.age_counts, plain.age_group_indices))
    if route == 'snapshot_default_groups':
        return _result(lambda: tx.report_from_snapshot(plain.snapshot(), plain.age_counts))
    return _result({'context_tree': a.transmission_report, 'context_tree_fine': lambda: a.transmission_report(tx_util.groups('fine')),
                    'log': log.report, 'log_40_days': lambda: log.report(n_days=40),
                    'lineage': log.lineage_report, 'lineage_by_day': lambda: log.lineage_report(1, None, tx_util.groups('fine')),
                    'lineage_30x1': lambda: log.lineage_report(30, 1),
                    'ensemble_tree': lambda: ensemble.transmission_reports([a, b]),
                    'ensemble_log': lambda: ensemble.log_reports([a, b]),
                    'ensemble_lineage': lambda: ensemble.lineage_reports([a, b], period=14),
                    'line_list': lambda: _line_list(a)}[route])


RUN = ('context_tree', 'context_tree_fine', 'log', 'log_40_days', 'lineage', 'lineage_by_day', 'lineage_30x1', 'snapshot',
       'snapshot_default_groups', 'ensemble_tree', 'ensemble_log', 'ensemble_lineage', 'line_list')


def _deep_case(route):
    c = _deep()
    first = tx.rounds_for(c.day + 1)
    out = _result({'tree': c.transmission_report, 'lineage': c.transmission_log.lineage_report,
                   'ensemble_tree': lambda: ensemble.transmission_reports([c, _runs()[0]]),
                   'ensemble_lineage': lambda: ensemble.lineage_reports([c, _runs()[0]], n_periods=9),
                   'line_list': lambda: _line_list(c)}[route])
    one = out[0] if isinstance(out, list) else out
    if 'scalars' in one:
        one['took_deep_pass'] = one['scalars']['rounds'] == tx.rounds_for(c.engine.config.n_agents) != first and one['scalars']['unconverged'] == 0
    return out


DEEP = ('tree', 'lineage', 'ensemble_tree', 'ensemble_lineage', 'line_list')


# ---------------------------------------------------------------------------------------------- refusals

def _refusal(name):
    a, b, plain = _runs()
    log = a.transmission_log
    n = 600
    hot, inf, cnt, words = tu.forest_state(n, 'random')
    age_start, g = tx_util.age_start_of(n), tx_util.groups()
    kind, _, value = name.rpartition('_')
    value = int(value)
    if kind == 'n_days':
        routes = dict(spec=lambda: txl.report_numpy(hot, inf, cnt, words, age_start, g, value),
                      log=lambda: log.report(n_days=value), ensemble=lambda: ensemble.log_reports([a, b], n_days=value))
    elif kind in ('period', 'n_periods'):
        args = (value, 5) if kind == 'period' else (7, value)
        routes = dict(spec=lambda: lin.report_numpy(hot, inf, cnt, words, age_start, g, *args),
                      report=lambda: lin.LineageReport(np.zeros(lin.report_words(5), dtype=np.uint64), *args),
                      log=lambda: log.lineage_report(*args), ensemble=lambda: ensemble.lineage_reports([a, b], *args))
    elif kind in ('ages', 'group'):
        table = tx_util.groups()[:value] if kind == 'ages' else np.full(tx_util.NR_AGES, value)
        routes = dict(spec_tree=lambda: tx.report_numpy(hot, inf, cnt, age_start, table),
                      spec_log=lambda: txl.report_numpy(hot, inf, cnt, words, age_start, table, 40),
                      spec_lineage=lambda: lin.report_numpy(hot, inf, cnt, words, age_start, table, 7, 5),
                      tree=lambda: a.transmission_report(table), log=lambda: log.report(table),
                      lineage=lambda: log.lineage_report(age_groups=table),
                      snapshot=lambda: tx.report_from_snapshot(plain.snapshot(), plain.age_counts, table),
                      ensemble_tree=lambda: ensemble.transmission_reports([a, b], table),
                      ensemble_log=lambda: ensemble.log_reports([a, b], table),
                      ensemble_lineage=lambda: ensemble.lineage_reports([a, b], age_groups=table))
    else:
        raise KeyError(name)
    return {route: _result(fn) for route, fn in routes.items()}


REFUSALS = ('n_days_0', 'n_days_4097', 'period_0', 'period_4097', 'n_periods_0', 'n_periods_257', 'ages_50', 'group_16')


CASES = {}
for _p in tx_util.PATTERNS:
    for _n in SIZES:
        for _d in (None, SHALLOW):
            CASES['forest-%s-%d-%s' % (_p, _n, 'all' if _d is None else 'shallow')] = functools.partial(_forest, _p, _n, _d)
for _s in SPECIAL:
    for _d in (None, SHALLOW):
        CASES['state-%s-%s' % (_s, 'all' if _d is None else 'shallow')] = functools.partial(_special, _s, _d)
CASES.update({'run-' + r: functools.partial(_run, r) for r in RUN})
CASES.update({'deep-' + r: functools.partial(_deep_case, r) for r in DEEP})
CASES.update({'refusal-' + r: functools.partial(_refusal, r) for r in REFUSALS})


@pytest.fixture(scope='module')
def expected():
    with open(WORDS) as f:
        return json.load(f)


def _reworded(want, value):
    """the recorded result with the texts of REWORDED (for the refused `value`) in place of the recorded ones"""
    if isinstance(want, list):
        return [_reworded(x, value) for x in want]
    if 'error' in want:
        kind, text = want['error']
        return dict(error=[kind, REWORDED[text].format(value) if text in REWORDED else text])
    if 'words' in want or 'sha256' in want:
        return want
    return {k: _reworded(v, value) for k, v in want.items()}


@pytest.mark.parametrize('name', sorted(CASES))
def test_every_report_has_the_words_it_had_before_the_shared_core(name, expected):
    got = json.loads(json.dumps(CASES[name]()))
    assert got == _reworded(expected[name], name.rpartition('_')[2])


def _leaves(x):
    if isinstance(x, list):
        for y in x:
            yield from _leaves(y)
    elif 'scalars' in x or 'error' in x or 'sha256' in x:
        yield x
    else:
        for y in x.values():
            yield from _leaves(y)


def test_the_recorded_cases_are_worth_comparing_with(expected):
    """among the recorded reports: bad links, agents left unconverged, a state with no infected agent, a report that took the
    deep pass; every refusal raised somewhere; all names of this file and no others"""
    assert sorted(expected) == sorted(CASES)
    reports = [x for case in expected.values() for x in _leaves(case) if 'scalars' in x]
    assert any(r['scalars'].get('bad_links', 0) > 0 for r in reports)
    assert any(r['scalars'].get('unconverged', 0) > 0 for r in reports)
    assert any(r['scalars'].get('n_infected_agents', r['scalars'].get('infected')) == 0 for r in reports)
    assert sum(bool(r.get('took_deep_pass')) for r in reports) >= 2             # the tree report's and the lineage report's
    tie = expected['state-two_largest_trees-all']
    assert tie['tree']['scalars']['largest_root'] == tie['lineage']['scalars']['largest_root'] == 2
    assert tie['tree']['scalars']['largest_cluster'] == 3
    assert expected['state-none_infected-all']['tree']['scalars']['largest_root'] == -1
    for name in REFUSALS:
        errors = [x for x in _leaves(expected['refusal-' + name]) if 'error' in x]
        assert errors and all(e['error'][0] == 'ValueError' for e in errors), name


class _NeverLaunched:
    """a device log that must not be asked for words"""

    def report_words(self, *args):
        raise AssertionError('report_group launched with an n_days out of range')


@pytest.mark.parametrize('n_days', (0, eng.MAX_DAYS + 1))
def test_report_group_refuses_n_days_out_of_range_like_the_single_route(n_days):
    """(the one knowing change of the shared core: before it, txlog.report_group handed such an n_days to the library)"""
    a, b, _ = _runs()
    with pytest.raises(ValueError) as group:
        txl.report_group(_NeverLaunched(), [a, b], None, n_days)
    with pytest.raises(ValueError) as single:
        a.transmission_log.report(n_days=n_days)
    assert str(group.value) == str(single.value) == 'n_days must be in [1, %d]' % eng.MAX_DAYS


if __name__ == '__main__':
    if '--record' in sys.argv:
        with open(WORDS, 'w') as f:
            json.dump({name: CASES[name]() for name in sorted(CASES)}, f, separators=(',', ':'), sort_keys=True)
            f.write('\n')
