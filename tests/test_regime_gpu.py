"""A policy and a log in one run, and the regime report, on the GPU (include/reina_regime.h): the device
route -- k_policy ahead of every day, the record launch behind it, one wait at the end -- against the host-driven logged policy
run on oracle B (policy.run_host_driven with a host-kept log: the specification), and k_regime_report against
regime.report_numpy on the read-back state.  Exact equality throughout.  The inputs are those of tests/regime_util.py;
tests/test_regime.py asserts on oracle B that they switch and cross the way these tests need."""
import collections
import ctypes
import functools

import numpy as np
import pytest

import policy_util as pu
import regime_util as ru
from par_backend import par_engine_factory
from reina_model_amd import engine as eng
from reina_model_amd import ensemble, policy as pol, regime as rgm, reports, simulation, txlog as txl

pytestmark = pytest.mark.gpu


def _gpu(seed=1, ages=None, variables=None, policy=None, **kw):
    v, mini_ages = ru.scenario()
    return simulation.make_context(v if variables is None else variables, age_counts=mini_ages if ages is None else ages, seed=seed,
                                   policy=ru.regime_policy() if policy is None else policy, **kw)


def _run_in(c, pieces, log_from=0):
    """DAYS days in `pieces`, both logs begun on day log_from (the start of a piece); returns the whole history and leaves the
    whole run's levels and mobility factors on the Context (policy_levels and mobility_history are the LAST piece's)"""
    hist, levels, mobility = [], [], []
    for n in pieces:
        if c.day == log_from and c.course_log is None:
            c.start_course_log()
        hist.append(c.run(n))
        levels.append(np.asarray(c.policy_levels))
        mobility += list(c.mobility_history)
    assert c.day == ru.DAYS and len(levels[-1]) == pieces[-1]
    c.policy_levels, c.mobility_history = np.concatenate(levels), mobility
    return np.concatenate(hist)


LATE = (ru.LATE_LOG_DAY, ru.DAYS - ru.LATE_LOG_DAY)


@functools.lru_cache(maxsize=None)
def _oracle(seed, late=False):
    """the specification: the host-driven logged policy run on oracle B, both logs from day 0 (late: from LATE_LOG_DAY)"""
    v, ages = ru.scenario()
    c = pu.make(v, ages, seed=seed, factory=par_engine_factory, policy=ru.regime_policy())
    hist = _run_in(c, LATE, ru.LATE_LOG_DAY) if late else _run_in(c, (ru.DAYS,))
    assert not c.transmission_log.on_device
    return c, hist


def _assert_logs(a, b, what=''):
    ru.assert_words(a.transmission_log.words(), b.transmission_log.words(), what + 'log')
    ru.assert_words(a.course_log.words(), b.course_log.words(), what + 'course')
    assert np.array_equal(a.policy_level_by_day, b.policy_level_by_day), what + 'levels by day'


def _assert_is_the_specification(dev, hist, late=False):
    ora, ho = _oracle(1, late)
    assert dev.transmission_log.on_device and dev.course_log.on_device and dev.engine.regime_f is not None
    pu.assert_same_run(dev, ora, hist, ho, planes=False)
    _assert_logs(dev, ora)


# ---------------------------------------------------------------------------------------------- 1. the device route is the specification

@pytest.mark.parametrize('form', ['hot', 'log'])
def test_run_equals_the_host_driven_run(form, monkeypatch):
    if form == 'log':
        monkeypatch.setenv('REINA_TXLOG_FORM', 'log')
    dev = _gpu(course=True)
    _assert_is_the_specification(dev, _run_in(dev, (ru.DAYS,)))


def test_run_plan_equals_the_host_driven_run():
    plan = _gpu().make_plan(ru.DAYS, policy=(p := ru.regime_policy()))
    dev = _gpu(policy=p, course=True)
    _assert_is_the_specification(dev, dev.run_plan(plan))


def test_stretches_equal_the_host_driven_run():
    dev = _gpu(course=True)
    _assert_is_the_specification(dev, _run_in(dev, ru.STRETCHES))


def test_a_log_begun_mid_run_equals_the_host_driven_run():
    dev = _gpu()
    _assert_is_the_specification(dev, _run_in(dev, LATE, ru.LATE_LOG_DAY), late=True)
    rep = dev.transmission_log.regime_report()
    ru.assert_words(rep.words, ru.spec_report(dev, rgm.policy_labels(dev, ru.DAYS), ru.DAYS).words, 'late log')
    assert rep == _oracle(1, True)[0].transmission_log.regime_report() and rep.dated < rep.infected


# ---------------------------------------------------------------------------------------------- 2. the logs observe and never steer

@pytest.fixture(scope='module')
def single():
    """one 160-day logged policy run on one engine: serves the report cases"""
    dev = _gpu(course=True)
    return dev, dev.run(ru.DAYS)


def test_the_logged_run_is_the_unlogged_run(single):
    dev, hist = single
    plain = _gpu()
    hp = plain.run(ru.DAYS)
    assert plain.transmission_log is None
    pu.assert_same_run(dev, plain, hist, hp, planes=True)


# ---------------------------------------------------------------------------------------------- 3. a group

@pytest.fixture(scope='module')
def group():
    v, ages = ru.scenario()
    return ensemble.run_policy_ensemble(v, ru.SEEDS, ru.DAYS, ru.regime_policy(), age_counts=ages, course=True)


def test_group_members_equal_their_single_runs(group):
    hist, levels, ctxs = group
    glog = reports.group_log(ctxs)
    assert glog is not None and glog.course is not None and glog.members == len(ru.SEEDS)
    for m, seed in enumerate(ru.SEEDS):
        ora, ho = _oracle(seed)
        assert np.array_equal(hist[m], ho), 'history of member %d' % m
        assert np.array_equal(levels[m], ora.policy_levels) and list(ctxs[m].mobility_history) == list(ora.mobility_history)
        _assert_logs(ctxs[m], ora, 'member %d: ' % m)
    assert len({pu.first_escalation(lv) for lv in levels}) > 1


def test_hus_group_equals_single_engines():
    v, p, seeds, days = pu.hus_variables(), pu.ward_policy(), [100, 101, 102, 103], pu.GROUP_HUS_DAYS
    hist, levels, ctxs = ensemble.run_policy_ensemble(v, seeds, days, p, course=True)
    for m, seed in enumerate(seeds):
        solo = simulation.make_context(v, seed=seed, policy=p, course=True)
        hs = solo.run(days)
        assert np.array_equal(hist[m], hs), 'history of member %d' % m
        assert np.array_equal(levels[m], solo.policy_levels)
        _assert_logs(ctxs[m], solo, 'member %d: ' % m)
        del solo
    assert levels.max() >= 1


# ---------------------------------------------------------------------------------------------- 5. - 8. the report

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


@pytest.mark.parametrize('name', sorted(ru.labellings(np.zeros(ru.DAYS))))
def test_device_report_equals_the_specification(single, name, calls):
    dev, _ = single
    labels, n_days = ru.labellings(dev.policy_levels)[name]
    rep = dev.transmission_log.regime_report(labels, n_days=n_days)
    assert calls == {'regime_report': 1}
    ru.assert_words(rep.words, ru.spec_report(dev, labels, n_days).words, name)
    assert rep.infected == 2242 and int(rep.days.sum()) == n_days and np.array_equal(rep.labels, labels)
    if name == 'levels':
        assert rep == dev.transmission_log.regime_report() == _oracle(1)[0].transmission_log.regime_report()


def test_one_launch_for_the_group_with_labels_per_member(group, calls):
    _, levels, ctxs = group
    cases = ru.labellings(levels[1])
    labels = [levels[0].astype(np.uint8), cases['modulo'][0], ru.labellings(levels[2])['fifth'][0]]
    reps = ensemble.regime_reports(ctxs, labels=labels)
    assert calls == {'group_regime_report': 1}
    for m, (c, r) in enumerate(zip(ctxs, reps)):
        ru.assert_words(r.words, ru.spec_report(c, labels[m], ru.DAYS).words, 'member %d' % m)
    assert reps[2].unlabelled > 0 and reps[0].unlabelled == 0
    own = ensemble.regime_reports(ctxs)
    for m, seed in enumerate(ru.SEEDS):
        assert own[m] == _oracle(seed)[0].transmission_log.regime_report()
    # a member taken alone: the specification on host copies
    calls.clear()
    assert ctxs[1].transmission_log.regime_report() == own[1] and not calls


@pytest.mark.parametrize('agents', ru.SMALL_POPULATIONS)
def test_tile_edges(agents):
    dev = _gpu(ages=ru.small_ages(agents), txlog=True)
    dev.run(ru.SMALL_DAYS)
    assert dev.engine.config.n_agents == agents
    rep = dev.transmission_log.regime_report()
    ru.assert_words(rep.words, ru.spec_report(dev, rgm.policy_labels(dev, ru.SMALL_DAYS), ru.SMALL_DAYS).words, '%d agents' % agents)
    assert rep.links > 100 and rep.links_crossing > 0


@pytest.mark.parametrize('name', ['levels', 'fifth'])
def test_ties_between_the_two_device_reports(single, name):
    dev, _ = single
    n_days = ru.DAYS + 40
    labels = np.full(n_days, rgm.NO_REGIME, dtype=np.uint8)
    labels[:ru.DAYS] = ru.labellings(dev.policy_levels)[name][0]
    ru.assert_ties(dev.transmission_log.regime_report(labels, n_days=n_days), dev.transmission_log.report(n_days=n_days))


# ---------------------------------------------------------------------------------------------- 9. the C ABI's refusals

def test_abi_refusals_leave_everything_as_it_was():
    ages, first, more = ru.small_ages(1535), 10, 10
    a, b, ref = [_gpu(ages=ages, course=True) for _ in range(3)]
    ref.run(first + more)
    for c in (a, b):
        c.run(first)
    members = [_gpu(seed=s, ages=ages) for s in (1, 2)]
    grp = eng.EngineGroup([c.engine for c in members])
    gpol = pol.DevicePolicy(a.policy, a.start_date, group=grp)
    glog = txl.DeviceLog(members[0].engine, group=grp)
    e, f, stream, torch = a.engine, a.engine.regime_f, a.engine.alloc.stream(), a.engine.alloc.torch
    pa, la, lb = pol._device_of(a)._h, a.transmission_log.device._h, b.transmission_log.device._h
    _, arr, n = _gpu(ages=ages).make_plan(2)['segments'][0]
    last = lambda: e.f['last_error']()
    words_before, course_before, trace_before = a.transmission_log.words(), a.course_log.words(), pol._device_of(a).read_trace(0, first)
    run, grun = f['policy_txlog_run_days'], f['group_policy_txlog_run_days']
    for fn, p, l, text in ((run, None, la, b'null'), (run, pa, None, b'null'), (grun, None, glog._h, b'null'),
                           (run, pa, lb, b'different engines'), (grun, gpol._h, glog._h, None), (grun, pa, la, b'made for one engine'),
                           (run, gpol._h, glog._h, b'made for a group'), (run, gpol._h, la, b'not of one kind'), (run, pa, glog._h, b'not of one kind')):
        if text is None:   # (the one valid pairing of the group's: refused for its bank, which was never uploaded)
            assert fn(p, l, arr, n, None, stream) == -1 and b'never uploaded' in last()
            continue
        assert fn(p, l, arr, n, None, stream) == -1 and text in last(), text
    assert run(pa, la, None, n, None, stream) == -1 and b'day list' in last()
    late = (eng.Day * 1)()
    late[0].day = eng.MAX_DAYS
    assert run(pa, la, late, 1, None, stream) == -1 and b'REINA_MAX_DAYS' in last()
    # the report
    UNTOUCHED = -77
    rep = torch.full((rgm.REPORT_WORDS + 2,), UNTOUCHED, dtype=torch.int64, device=e.alloc.device)
    table = np.zeros(eng.MAX_AGES, dtype=np.uint8)
    labels = np.zeros(first, dtype=np.uint8)
    report, greport = f['regime_report'], f['group_regime_report']
    ptr = lambda x: ctypes.c_void_p(x.ctypes.data)
    assert report(None, ptr(table), 1, first, ptr(labels), rep.data_ptr(), stream) == -1
    assert greport(la, ptr(table), 1, first, ptr(labels), rep.data_ptr(), stream) == -1 and b'made for one engine' in last()
    assert report(glog._h, ptr(table), 1, first, ptr(labels), rep.data_ptr(), stream) == -1 and b'made for a group' in last()
    for n_days in (0, eng.MAX_DAYS + 1):
        assert report(la, ptr(table), 1, n_days, ptr(labels), rep.data_ptr(), stream) == -1
        assert b'regime report: n_days must be in [1, REINA_MAX_DAYS]' in last()
    assert report(la, None, 1, first, ptr(labels), rep.data_ptr(), stream) == -1 and b'regime report: age_group' in last()
    assert report(la, ptr(table), 1, first, ptr(labels), rep.data_ptr() + 8, stream) == -1
    assert b'regime report: the report must be a 16-byte aligned device buffer' in last()
    # (the labels are looked at last)
    assert report(la, ptr(table), 1, first, None, rep.data_ptr(), stream) == -1 and b'labels is null' in last()
    eight = labels.copy()
    eight[first - 1] = 8
    assert report(la, ptr(table), 1, first, ptr(eight), rep.data_ptr(), stream) == -1 and b'a label is neither' in last()
    torch.cuda.synchronize()
    assert bool((rep == UNTOUCHED).all()), 'a refused call queued something'
    # nothing has moved: the log, the course, the trace -- and a following valid run and report
    ru.assert_words(a.transmission_log.words(), words_before, 'log')
    ru.assert_words(a.course_log.words(), course_before, 'course')
    assert np.array_equal(pol._device_of(a).read_trace(0, first), trace_before)
    a.run(more)
    _assert_logs(a, ref)
    assert report(la, ptr(table), 1, first, ptr(labels), rep.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    got = rep.cpu().numpy()
    want = rgm.report_numpy(*ru.state(a), a.age_start, np.zeros(a.nr_ages, dtype=np.int64), labels, first)
    ru.assert_words(got[:rgm.REPORT_WORDS].view(np.uint64), want.words, 'the valid report')
    assert (got[rgm.REPORT_WORDS:] == UNTOUCHED).all(), 'the block is REPORT_WORDS words'
    gpol.close()
    glog.close()
    grp.close()
