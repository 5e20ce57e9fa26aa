"""How many device calls each route of a report of a log makes (reina_model_amd/reports.py: the three routes).  The words cannot
show it: a group route turned into one call per member, or a single call made twice, gives the same reports.  The counts are
literals, taken from a run of this file on commit 88d6790, before the routes were stated once."""
import collections
import gc

import pytest

import tx_util
import txlog_util as tu
from filter_util import small_scenario
from reina_model_amd import ensemble, reports, simulation

pytestmark = pytest.mark.gpu

N, DAYS, MEMBERS = 700, 12, 4
FOUR = dict(log=ensemble.log_reports, lineage=ensemble.lineage_reports, course=ensemble.course_reports,
            vaccination=ensemble.vaccination_reports)


@pytest.fixture(autouse=True)
def _engines_go_with_their_test():
    """(a logged Context and its log refer to each other: tests/test_filter_log_gpu.py)"""
    yield
    gc.collect()


@pytest.fixture
def calls(monkeypatch):
    """{entry-point name: calls} of reports.device_words from here on"""
    seen = collections.Counter()
    inner = reports.device_words

    def counting(engine, f, name, *args, **kw):
        seen[name] += 1
        return inner(engine, f, name, *args, **kw)

    monkeypatch.setattr(reports, 'device_words', counting)
    return seen


def _make(seed, **kw):
    v, ages = small_scenario(N)
    return simulation.make_context(v, age_counts=ages, seed=seed, ipc='auto', **kw)


def _taken(calls, fn):
    calls.clear()
    reps = fn()
    return reps, dict(calls)


def test_a_whole_group_is_one_call_and_members_on_their_own_are_none(calls):
    planner = _make(11)
    ctxs = [_make(11 + m) for m in range(MEMBERS)]
    ensemble.run_group_plan(ctxs, planner.make_plan(DAYS), txlog=True, course=True)
    glog = ctxs[0].transmission_log.device
    try:
        got = {what: _taken(calls, lambda: fn(ctxs)) for what, fn in FOUR.items()}
        assert all(len(reps) == MEMBERS for reps, _ in got.values())
        assert {what: n for what, (_, n) in got.items()} == dict(
            log={'group_txlog_report': 1}, lineage={'group_lineage_report': 1}, course={'course_report': 1},
            vaccination={'vacc_report': 1})
        some = [ctxs[0], ctxs[2]]         # not the whole group: one by one, numpy on read-back
        part = {what: _taken(calls, lambda: fn(some)) for what, fn in FOUR.items()}
        assert all(len(reps) == 2 for reps, _ in part.values())
        assert {what: n for what, (_, n) in part.items()} == dict(log={}, lineage={}, course={}, vaccination={})
        for what in FOUR:                 # (and they are the reports the launch gave those members)
            assert part[what][0] == [got[what][0][0], got[what][0][2]], what
    finally:
        for c in ctxs:
            c.transmission_log = c.course_log = None
        group = glog.group
        glog.close()
        group.close()


def test_a_device_log_of_its_own_is_one_call(calls):
    c = _make(5, txlog=True, course=True)
    c.run(DAYS)
    log = c.transmission_log
    assert log.on_device and c.course_log.on_device
    single = dict(log=log.report, lineage=log.lineage_report, course=c.course_log.report, vaccination=log.vaccination_report)
    assert {what: _taken(calls, fn)[1] for what, fn in single.items()} == dict(
        log={'txlog_report': 1}, lineage={'lineage_report': 1}, course={'course_report': 1}, vaccination={'vacc_report': 1})
    listed = {what: _taken(calls, lambda: fn([c]))[1] for what, fn in FOUR.items()}   # (a list of one: the same single route)
    assert listed == dict(log={'txlog_report': 1}, lineage={'lineage_report': 1}, course={'course_report': 1},
                          vaccination={'vacc_report': 1})
    c.course_log.close()
    log.close()


def test_the_deep_lineage_pass_is_a_second_call(calls):
    """a chain of 300 on a Context of three days, as tests/test_reports_words.py's _deep: deeper than its day + 1"""
    c = _make(9, txlog=True)
    n = c.engine.config.n_agents
    tx_util.put_forest(c, *tx_util.forest(n, 'chain', size=300), day=3)
    c.day = 3
    c.transmission_log.set_words(tu.random_log(n, top=3))
    rep, seen = _taken(calls, c.transmission_log.lineage_report)
    assert seen == {'lineage_report': 2}
    assert rep.unconverged == 0 and rep.rounds == tx_util.tx.rounds_for(n) != tx_util.tx.rounds_for(c.day + 1)
    c.transmission_log.close()
