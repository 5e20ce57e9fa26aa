"""The dated transmission log on the GPU: the device route (k_txlog_begin once, k_txlog_day behind every day, k_txlog_report)
against the plain formulation (txlog.run_host_driven: iterate, read the hot words back, record_numpy) and against the numpy
specification of the report.  Exact equality throughout; the simulated runs are shared between the tests through
module-scoped fixtures."""
import copy
import ctypes

import numpy as np
import pytest

import snap_util
import tx_util
import txlog_util as tu
from filter_util import assert_same_day_state, small_scenario
from reina_model_amd import datasets, ensemble, simulation, sharding, txlog as txl
from reina_model_amd import engine as eng
from reina_model_amd.variables import VARIABLE_DEFAULTS

pytestmark = pytest.mark.gpu

IPC = dict(dead=2, in_icu=1, in_ward=3, confirmed_cases=20, infected_cases=40, incubating=15, ill=10, recovered=10)   # tests/test_snapshot.py's
HUS_DAYS, MINI_DAYS = 200, 200
GROUP_SEEDS = list(range(200, 216))
GROUP_DAYS = 120


def _make(v, ages=None, seed=1, ipc='auto', txlog=False, snapshot=None):
    return simulation.make_context(v, age_counts=ages, seed=seed, ipc=ipc, txlog=txlog, snapshot=snapshot)


def _hus():
    return copy.deepcopy(VARIABLE_DEFAULTS)


def _same_words(got, want, what='log'):
    got, want = np.asarray(got), np.asarray(want)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, '%s: %d words differ, first agent %d: %#x != %#x' % (what, len(bad), bad[0], got[bad[0]], want[bad[0]])


def _same_history(ha, hb, what='history'):
    bad = np.argwhere(np.asarray(ha) != np.asarray(hb))
    assert len(bad) == 0, '%s: %d words differ, first at %s' % (what, len(bad), bad[0])


def _plane_check(ctx):
    """after every host-driven day: the ACTIVE bit plane on the device == the hot words' ACTIVE flags (what k_txlog_day streams)"""
    n = ctx.engine.config.n_agents

    def check(day, hot):
        plane = ctx.engine.tensors['active_bits'].cpu().numpy().view(np.uint32)
        bits = np.unpackbits(plane.view(np.uint8), bitorder='little')
        want = (hot & tu.ACTIVE) != 0
        assert np.array_equal(bits[:n].astype(bool), want), 'day %d: the ACTIVE plane differs from the hot words' % day
        assert not bits[n:].any(), 'day %d: bits beyond the population' % day
    return check


def _host_driven(v, ages, seed, days, ipc='auto', planes=True):
    host = _make(v, ages, seed, ipc)
    facts = tu.DayFacts(_plane_check(host) if planes else None)
    hist = txl.run_host_driven(host, days, on_day=facts)
    assert host.transmission_log is not None and not host.transmission_log.on_device
    return host, hist, facts


def _device_and_host(v, ages, seed, days, ipc='auto'):
    dev = _make(v, ages, seed, ipc, txlog=True)
    assert dev.engine.txlog_f is not None and dev.transmission_log.on_device
    hd = dev.run(days)
    host, hh, facts = _host_driven(v, ages, seed, days, ipc)
    _same_history(hd, hh)
    _same_words(dev.transmission_log.words(), host.transmission_log.words())
    return dev, hd, host, facts


def _report_equals_spec(ctx, n_days=None, groups=None):
    got = ctx.transmission_log.report(groups, n_days)
    want = tu.spec_report(ctx, ctx.transmission_log.words(), n_days, groups)
    tu.assert_words(got.words, want.words)
    return got


# ---------------------------------------------------------------------------------------------- 5. device log == host-driven log

@pytest.fixture(scope='module')
def hus_200():
    dev, hd, host, facts = _device_and_host(_hus(), None, 5, HUS_DAYS)
    host_words = host.transmission_log.words()
    del host
    return dev, hd, host_words, facts


@pytest.fixture(scope='module')
def mini_200():
    v, ages = small_scenario()
    dev, hd, host, facts = _device_and_host(v, ages, 3, MINI_DAYS)
    return dev, hd, host.transmission_log.words(), facts


def test_hus_200_days_device_log_equals_host_driven(hus_200):
    dev, hd, host_words, facts = hus_200
    r = _report_equals_spec(dev)
    assert r.dated == sum(facts.dated.values()) > 300000 and r.generation_nonpositive == 0 and r.out_of_range == 0
    assert r.with_onset == sum(facts.onsets.values())


def test_mini_200_days_device_log_equals_host_driven(mini_200):
    dev, hd, host_words, facts = mini_200
    r = _report_equals_spec(dev)
    assert r.dated == sum(facts.dated.values()) > 5000
    _report_equals_spec(dev, n_days=50)          # (most dated values out of range)
    _report_equals_spec(dev, n_days=eng.MAX_DAYS, groups=np.minimum(np.arange(101) // 7, 15))
    ll = dev.transmission_log.line_list()
    assert len(ll) == r.infected and int((ll['infection_day'] >= 0).sum()) == r.dated


def test_initial_condition_on_the_device_keeps_before():
    """the trap of day 0: the initial condition's incubating agents carry day 0 in bits 24-31 and must stay BEFORE"""
    v, ages = small_scenario()
    dev, hd, host, facts = _device_and_host(v, ages, 5, 120, ipc=IPC)
    words = dev.transmission_log.words()
    r = _report_equals_spec(dev)
    assert r.before == int(((words & 0xFFFF) == txl.BEFORE).sum()) >= IPC['incubating']


def test_ten_million_agents_60_days():
    v = _hus()
    ages = datasets.scaled_population(10 ** 7)
    dev, hd, host, facts = _device_and_host(v, ages, 7, 60)
    r = _report_equals_spec(dev)
    assert r.dated == sum(facts.dated.values()) > 0


@pytest.mark.parametrize('mode', ('dense', 'sparse', 'alternate'))
def test_mini_under_every_day_mode(mode, mini_200, monkeypatch):
    monkeypatch.setenv('REINA_DAY_MODE', mode)
    v, ages = small_scenario()
    dev = _make(v, ages, 3, txlog=True)
    hd = dev.run(MINI_DAYS)
    _same_history(hd, mini_200[1])
    _same_words(dev.transmission_log.words(), mini_200[2])


def test_mini_with_the_log_word_form_of_the_day_kernel(mini_200, monkeypatch):
    monkeypatch.setenv('REINA_TXLOG_FORM', 'log')
    v, ages = small_scenario()
    dev = _make(v, ages, 3, txlog=True)
    dev.run(MINI_DAYS)
    _same_words(dev.transmission_log.words(), mini_200[2])


def test_four_stretches_and_strict_iterate_equal_one_run(mini_200):
    v, ages = small_scenario()
    a = _make(v, ages, 3, txlog=True)
    hist = np.concatenate([a.run(n) for n in (1, 59, 100, 40)])
    _same_history(hist, mini_200[1])
    _same_words(a.transmission_log.words(), mini_200[2])
    b = simulation.make_context(v, age_counts=ages, seed=3, ipc='auto', strict=True, txlog=True)
    for _ in range(MINI_DAYS):
        b.iterate()
    _same_words(b.transmission_log.words(), mini_200[2])
    assert_same_day_state(a, b)


# ---------------------------------------------------------------------------------------------- 6. a logged run == the plain run

def test_logged_run_computes_what_the_plain_run_computes(hus_200, mini_200):
    for (dev, hd, _, _), v, ages, seed, days in ((hus_200, _hus(), None, 5, HUS_DAYS), (mini_200,) + small_scenario() + (3, MINI_DAYS)):
        plain = _make(v, ages, seed)
        hp = plain.run(days)
        _same_history(hd, hp)
        assert_same_day_state(dev, plain)
        del plain


# ---------------------------------------------------------------------------------------------- 7. device report == report_numpy

def _synthetic_case(hot, inf, cnt, log, kind='default', n_days=tu.N_DAYS):
    n = len(hot)
    ctx = snap_util.make_context(n)
    tx_util.put_forest(ctx, hot, inf, cnt)
    tlog = ctx.start_transmission_log()
    tlog.set_words(log)
    _same_words(tlog.words(), log, 'written log')
    g = tx_util.groups(kind)
    got = tlog.report(g, n_days)
    want = txl.report_numpy(hot, inf, cnt, log, np.asarray(ctx.engine.config.age_start), g, n_days)
    tu.assert_words(got.words, want.words)
    return got


@pytest.mark.parametrize('n', tu.SIZES)
@pytest.mark.parametrize('pattern', tx_util.PATTERNS)
def test_report_kernel_equals_spec_on_forests(pattern, n):
    _synthetic_case(*tu.forest_state(n, pattern), kind='fine' if n % 2 else 'default')


def test_report_kernel_equals_spec_on_every_code_combination():
    st = tu.combos_state()
    r = _synthetic_case(*st)
    assert r.generation_nonpositive >= 2 and r.bad_links == 1 and r.out_of_range == 5
    _synthetic_case(*st, n_days=1)
    _synthetic_case(*st, n_days=eng.MAX_DAYS)


def test_report_kernel_equals_spec_on_a_large_forest():
    r = _synthetic_case(*tu.forest_state(3_000_000, 'random'))
    assert r.links > 10 ** 6 and r.out_of_range > 0
    _synthetic_case(*tu.forest_state(3_000_000, 'bad_links'), kind='fine')


def test_begin_pass_equals_begin_numpy_at_tile_edges():
    for n in tu.SIZES:
        hot, inf, cnt = tx_util.forest(n, 'random', seed=n)
        ctx = snap_util.make_context(n)
        tx_util.put_forest(ctx, hot, inf, cnt)
        _same_words(ctx.start_transmission_log().words(), txl.begin_numpy(hot), 'begin pass, n = %d' % n)


# ---------------------------------------------------------------------------------------------- 8. groups

def _group_against_singles(v, ages, seeds, days):
    planner = _make(v, ages, seeds[0])
    ctxs = [_make(v, ages, sd) for sd in seeds]
    hist = ensemble.run_group_plan(ctxs, planner.make_plan(days // 2), txlog=True)
    hist = np.concatenate([hist, ensemble.run_group_plan(ctxs, planner.make_plan(days - days // 2))], axis=1)   # (the logs continue)
    reps = ensemble.log_reports(ctxs)
    assert len(reps) == len(seeds)
    for m, sd in enumerate(seeds):
        solo = _make(v, ages, sd, txlog=True)
        hs = solo.run(days)
        _same_history(hist[m], hs, 'member %d' % m)
        _same_words(ctxs[m].transmission_log.words(), solo.transmission_log.words(), 'member %d' % m)
        tu.assert_words(reps[m].words, solo.transmission_log.report().words)
        tu.assert_words(reps[m].words, ctxs[m].transmission_log.report().words)   # (a member's own report: the numpy route)
        if m % 8 == 0:
            assert_same_day_state(ctxs[m], solo)
        del solo
    return reps


def test_sixteen_hus_members_as_one_logged_group():
    reps = _group_against_singles(_hus(), None, GROUP_SEEDS, GROUP_DAYS)
    assert len(set(r.dated for r in reps)) > 1


@pytest.mark.parametrize('members', (1, 3))
def test_ragged_logged_groups(members):
    v, ages = small_scenario()
    _group_against_singles(v, ages, list(range(40, 40 + members)), 90)


# ---------------------------------------------------------------------------------------------- 9. logs begun mid-run

def test_log_begun_at_day_60_and_after_a_restore_at_day_120(mini_200):
    v, ages = small_scenario()
    full = mini_200[2]
    ft, fo = full & 0xFFFF, full >> 16

    def tail(cut):
        return np.where(fo < cut, txl.BEFORE, fo).astype(np.uint32) << 16 | np.where(ft < cut, txl.BEFORE, ft).astype(np.uint32)

    a = _make(v, ages, 3)
    a.run(60)
    a.start_transmission_log()
    a.run(MINI_DAYS - 60)
    _same_words(a.transmission_log.words(), tail(60), 'begun at day 60')
    _report_equals_spec(a)
    b = _make(v, ages, 3)
    b.run(120)
    snap = b.snapshot()
    c = _make(v, ages, 3, snapshot=snap, txlog=True)
    assert c.day == 120 and c.transmission_log.begin_day == 120
    c.run(MINI_DAYS - 120)
    _same_words(c.transmission_log.words(), tail(120), 'begun on a restored Context')


# ---------------------------------------------------------------------------------------------- 10. refusals

def test_refusals():
    v, ages = small_scenario()
    for attribution in ('exact', 'mirror'):
        members = []
        shards = [simulation.make_context(v, age_counts=ages, seed=1, ipc=None, comm=sharding.InProcessComm(r, 2, members, attribution=attribution))
                  for r in range(2)]
        e = shards[0].engine
        h = ctypes.c_void_p()
        assert e.txlog_f['txlog_create'](e._h, e.alloc.stream(), ctypes.byref(h)) == -1 and not h
        assert b'sharded' in e.f['last_error']()
        with pytest.raises(ValueError, match='sharded'):
            shards[0].start_transmission_log()
        del shards, members
    c = _make(v, ages, 1, txlog=True)
    e, log = c.engine, c.transmission_log.device
    assert log.f['txlog_record_day'](log._h, eng.MAX_DAYS, e.alloc.stream()) == -1 and b'REINA_MAX_DAYS' in e.f['last_error']()
    rep = e.alloc.torch.zeros(txl.report_words(4), dtype=e.alloc.torch.int64, device=e.alloc.device)
    table = np.zeros(eng.MAX_AGES, dtype=np.uint8)
    for n_days in (0, eng.MAX_DAYS + 1):
        assert log.f['txlog_report'](log._h, table.ctypes.data, 1, n_days, rep.data_ptr(), e.alloc.stream()) == -1
        assert b'n_days' in e.f['last_error']()
    # a single engine's log through the group entry points, and the other way round
    assert log.f['group_txlog_report'](log._h, table.ctypes.data, 1, 4, rep.data_ptr(), e.alloc.stream()) == -1
    assert log.f['group_txlog_run_days'](log._h, (eng.Day * 1)(), 0, None, e.alloc.stream()) == -1
    ctxs = [_make(v, ages, sd) for sd in (1, 2)]
    group = eng.EngineGroup([x.engine for x in ctxs])
    glog = txl.DeviceLog(ctxs[0].engine, group=group)
    assert glog.f['txlog_report'](glog._h, table.ctypes.data, 1, 4, rep.data_ptr(), e.alloc.stream()) == -1
    assert glog.f['txlog_run_days'](glog._h, (eng.Day * 1)(), 0, None, e.alloc.stream()) == -1
    assert b'group' in e.f['last_error']()
    glog.close()
    group.close()
    with pytest.raises(ValueError, match='transmission log'):
        c.snapshot()
    from reina_model_amd import filtering
    with pytest.raises(ValueError, match='transmission log'):
        filtering.FilterResult(c, [c], None, 0, c.start_date, 0)
