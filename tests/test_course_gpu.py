"""The clinical course log on the GPU: the device route (k_course_begin once, k_course_day in the transmission log's launch of
every day, k_course_report) against the plain formulation (course.run_host_driven: iterate, read the hot words back,
record_numpy) and against the numpy specification of the report.  Exact equality throughout; the simulated runs are shared
between the tests through module-scoped fixtures."""
import copy
import ctypes

import numpy as np
import pytest

import course_util as cu
import snap_util
import tx_util
import txlog_util as tu
from filter_util import assert_same_day_state, small_scenario
from reina_model_amd import course as crs
from reina_model_amd import engine as eng
from reina_model_amd import ensemble, simulation, sharding, txlog as txl
from reina_model_amd.variables import VARIABLE_DEFAULTS

pytestmark = pytest.mark.gpu

DAYS = 200


def _make(v, ages=None, seed=1, ipc='auto', **kw):
    return simulation.make_context(v, age_counts=ages, seed=seed, ipc=ipc, **kw)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert len(bad) == 0, '%s: %d words differ, first at %s: %#x != %#x' % (what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


def _hot(ctx):
    return ctx.engine.tensors['hot'].cpu().numpy().view(np.uint32)


def _report_equals_spec(ctx, n_days=None, groups=None):
    got = ctx.course_log.report(groups, n_days)
    table = ctx._tx_groups(groups)[0]
    want = crs.report_numpy(_hot(ctx), ctx.transmission_log.words(), ctx.course_log.words(), ctx.age_start, table,
                            max(ctx.day, 1) if n_days is None else n_days)
    cu.assert_words(got.words, want.words)
    return got


class Reference:
    """one scenario three ways: host-driven with log and course (the plain formulation), and the plain run without either"""

    def __init__(self, v, ages, seed, days, ipc='auto'):
        host = _make(v, ages, seed, ipc)
        self.hist = crs.run_host_driven(host, days)
        assert not host.transmission_log.on_device and not host.course_log.on_device
        self.log, self.rec = host.transmission_log.words(), host.course_log.words()
        self.plain = _make(v, ages, seed, ipc)
        _same(self.plain.run(days), self.hist, 'plain history')
        assert_same_day_state(host, self.plain)

    def check(self, dev, hist, what):
        assert dev.course_log.on_device and dev.transmission_log.on_device and dev.engine.course_f is not None
        if hist is not None:
            _same(hist, self.hist, what + ': history')
        _same(dev.course_log.words(), self.rec, what + ': records')
        _same(dev.transmission_log.words(), self.log, what + ': log words')
        assert_same_day_state(dev, self.plain)
        return _report_equals_spec(dev)


@pytest.fixture(scope='module')
def mini():
    v, ages = small_scenario()
    return Reference(v, ages, 3, DAYS)


# ---------------------------------------------------------------------------------------------- device == host-driven

@pytest.mark.parametrize('env', ('REINA_DAY_MODE=dense', 'REINA_DAY_MODE=sparse', 'REINA_DAY_MODE=alternate', 'REINA_TXLOG_FORM=log', ''))
def test_mini_200_days_device_course_equals_host_driven(env, mini, monkeypatch):
    if env:
        monkeypatch.setenv(*env.split('='))
    v, ages = small_scenario()
    dev = _make(v, ages, 3, course=True)
    r = mini.check(dev, dev.run(DAYS), env or 'default')
    assert r.with_admission > 50 and r.with_outcome > 5000 and r.out_of_range == 0 and int(r.pathway[:, 9].sum()) == 0
    if not env:
        _report_equals_spec(dev, n_days=50)          # (most known days out of range)
        _report_equals_spec(dev, n_days=eng.MAX_DAYS, groups=np.minimum(np.arange(101) // 7, 15))
        ll = dev.transmission_log.line_list()
        assert int((ll['admission_day'] >= 0).sum()) == r.with_admission and int((ll['outcome_day'] >= 0).sum()) == r.with_outcome


def test_four_stretches_and_strict_iterate_equal_one_run(mini):
    v, ages = small_scenario()
    a = _make(v, ages, 3, course=True)
    mini.check(a, np.concatenate([a.run(n) for n in (1, 59, 100, 40)]), 'four stretches')
    b = _make(v, ages, 3, strict=True, course=True)
    for _ in range(DAYS):
        b.iterate()
    mini.check(b, None, 'strict iterate')


def test_initial_condition_on_the_device():
    v, ages = small_scenario()
    ref = Reference(v, ages, 5, 120, ipc=cu.IPC)
    dev = _make(v, ages, 5, ipc=cu.IPC, course=True)
    r = ref.check(dev, dev.run(120), 'initial condition')
    assert int(r.pathway[:, 9].sum()) >= cu.IPC['dead'] + cu.IPC['recovered'] + cu.IPC['in_icu'] + cu.IPC['in_ward']


def test_hus_200_days_device_course_equals_host_driven():
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    ref = Reference(v, None, 5, DAYS)
    dev = _make(v, None, 5, course=True)
    r = ref.check(dev, dev.run(DAYS), 'HUS')
    assert r.with_outcome > 100000 and r.with_admission > 1000 and r.out_of_range == 0


# ---------------------------------------------------------------------------------------------- synthetic states

def _synthetic(hot, inf, cnt):
    ctx = snap_util.make_context(len(hot))
    tx_util.put_forest(ctx, hot, inf, cnt)
    course = ctx.start_course_log()
    assert course.on_device
    return ctx, course


def _synthetic_report(ctx, hot, log, rec, n_days, kind='default'):
    g = tx_util.groups(kind)
    got = ctx.course_log.report(g, n_days)
    want = crs.report_numpy(hot, log, rec, np.asarray(ctx.engine.config.age_start), g, n_days)
    cu.assert_words(got.words, want.words)
    return got


@pytest.mark.parametrize('n', tu.SIZES)
def test_begin_and_report_kernels_equal_spec_at_tile_edges(n):
    hot, inf, cnt, log, rec = cu.forest_state(n)
    ctx, course = _synthetic(hot, inf, cnt)
    _same(course.words(), crs.begin_numpy(hot), 'begin pass')
    begin = course.words()
    _synthetic_report(ctx, hot, ctx.transmission_log.words(), begin, cu.N_DAYS)
    course.set_words(rec)
    ctx.transmission_log.set_words(log)
    _same(course.words(), rec, 'written records')
    _synthetic_report(ctx, hot, log, rec, cu.N_DAYS, 'fine' if n % 2 else 'default')


def test_report_kernel_equals_spec_on_every_code_combination():
    hot, inf, cnt, log, rec = cu.combos_state()
    ctx, course = _synthetic(hot, inf, cnt)
    _same(course.words(), crs.begin_numpy(hot), 'begin pass')
    course.set_words(rec)
    ctx.transmission_log.set_words(log)
    r = _synthetic_report(ctx, hot, log, rec, cu.N_DAYS)
    assert (r.pathway.sum(axis=0) > 0).all() and (r.delay_n.sum(axis=1) > 0).all() and r.out_of_range > 0 and r.detected_undated > 0
    _synthetic_report(ctx, hot, log, rec, 1)
    _synthetic_report(ctx, hot, log, rec, eng.MAX_DAYS, 'fine')


def _put_active_plane(ctx, hot):
    """the ACTIVE bit plane of a synthetic state (what k_course_day streams), from its hot words"""
    import torch
    t = ctx.engine.tensors['active_bits']
    plane = np.zeros(t.numel(), dtype=np.uint32)
    packed = np.packbits((hot & cu.ACTIVE) != 0, bitorder='little')
    plane.view(np.uint8)[:len(packed)] = packed
    t.copy_(torch.from_numpy(plane.view(np.int32)))


@pytest.mark.parametrize('state', ('combos', 'forest'))
def test_day_kernel_equals_record_numpy_on_synthetic_states(state):
    hot, inf, cnt, log, rec = cu.combos_state() if state == 'combos' else cu.forest_state(tu.SIZES[-1], seed=4)
    if state == 'forest':   # (plant agents whose bits 24-31 say "infected today" and "onset today" of the days recorded below)
        ill = np.flatnonzero((hot & 7) == 2)[:40]
        hot[ill] = (hot[ill] & 0x00FFFFFF) | np.uint32(132 << 24) | cu.ACTIVE
        inc = np.flatnonzero((hot & 7) == 1)[:40]
        hot[inc] = (hot[inc] & 0x00FFFFFF) | np.uint32(131 << 24) | cu.ACTIVE
    ctx, course = _synthetic(hot, inf, cnt)
    _put_active_plane(ctx, hot)
    course.set_words(rec)
    ctx.transmission_log.set_words(log)
    active = (hot & cu.ACTIVE) != 0
    rec0 = rec
    dlog = ctx.transmission_log.device
    # the first day a log records: the form that reads the log word; then the day that follows it: the hot-word form; then a
    # day after a gap: the log-word form again
    for day, by_hot in ((130, False), (131, True), (140, False)):
        dlog.record_day(day)
        rec = crs.record_numpy(rec, hot, day, where=active)
        log = tu.record_by_hot(log, hot, day) if by_hot else np.where(active, txl.record_numpy(log, hot, day), log)
        _same(course.words(), rec, 'day %d: records' % day)
        _same(ctx.transmission_log.words(), log, 'day %d: log words' % day)
    closed_on = lambda day: int(((crs.fields(rec)[3] == day) & (crs.fields(rec0)[3] == txl.NONE)).sum())
    assert closed_on(130) > 0 and closed_on(131) == closed_on(140) == 0, 'the removed agents closed on the first day recorded'
    _same(_hot(ctx), hot, 'hot words')


# ---------------------------------------------------------------------------------------------- groups

@pytest.mark.parametrize('members', (1, 3, 4))
def test_coursed_groups_equal_single_contexts(members):
    v, ages = small_scenario()
    seeds, days = list(range(40, 40 + members)), 90
    planner = _make(v, ages, seeds[0])
    ctxs = [_make(v, ages, sd) for sd in seeds]
    hist = ensemble.run_group_plan(ctxs, planner.make_plan(days // 2), txlog=True, course=True)
    hist = np.concatenate([hist, ensemble.run_group_plan(ctxs, planner.make_plan(days - days // 2))], axis=1)   # (the logs continue)
    reps = ensemble.course_reports(ctxs)
    assert len(reps) == members and all(c.course_log.device is ctxs[0].course_log.device for c in ctxs)
    for m, sd in enumerate(seeds):
        solo = _make(v, ages, sd, course=True)
        _same(hist[m], solo.run(days), 'member %d: history' % m)
        _same(ctxs[m].course_log.words(), solo.course_log.words(), 'member %d: records' % m)
        _same(ctxs[m].transmission_log.words(), solo.transmission_log.words(), 'member %d: log words' % m)
        cu.assert_words(reps[m].words, solo.course_log.report().words)
        cu.assert_words(reps[m].words, ctxs[m].course_log.report().words)   # (a member's own report: the numpy route)
        assert_same_day_state(ctxs[m], solo)
        del solo
    assert reps[0].with_outcome > 0


# ---------------------------------------------------------------------------------------------- courses begun mid-run

def test_course_begun_at_day_60_and_on_a_restored_context_at_day_120(mini):
    v, ages = small_scenario()
    a = _make(v, ages, 3)
    a.run(60)
    hot60 = _hot(a).copy()
    a.start_course_log()
    assert a.transmission_log is not None and a.course_log.begin_day == 60
    a.run(DAYS - 60)
    _same(a.course_log.words(), cu.cut_records(mini.rec, 60, hot60), 'begun at day 60')
    r = _report_equals_spec(a)
    assert int(r.pathway[:, 9].sum()) > 0
    b = _make(v, ages, 3)
    b.run(120)
    hot120 = _hot(b).copy()
    c = _make(v, ages, 3, snapshot=b.snapshot(), course=True)
    assert c.day == 120 and c.course_log.begin_day == 120 and c.course_log.on_device
    c.run(DAYS - 120)
    _same(c.course_log.words(), cu.cut_records(mini.rec, 120, hot120), 'begun on a restored Context')
    _report_equals_spec(c)


# ---------------------------------------------------------------------------------------------- refusals

def test_refusals():
    v, ages = small_scenario()
    members = []
    shards = [simulation.make_context(v, age_counts=ages, seed=1, ipc=None, comm=sharding.InProcessComm(r, 2, members)) for r in range(2)]
    e = shards[0].engine
    h, hc = ctypes.c_void_p(), ctypes.c_void_p()
    assert e.txlog_f['txlog_create'](e._h, e.alloc.stream(), ctypes.byref(h)) == -1 and not h      # (a sharded engine gets no log ...)
    assert e.course_f['course_create'](h, e.alloc.stream(), ctypes.byref(hc)) == -1 and not hc     # (... and so no course)
    with pytest.raises(ValueError, match='sharded'):
        shards[0].start_course_log()
    assert shards[0].course_log is None
    del shards, members
    c = _make(v, ages, 1, course=True)
    e, course = c.engine, c.course_log.device
    f = course.f
    assert f['course_create'](c.transmission_log.device._h, e.alloc.stream(), ctypes.byref(hc)) == -1 and not hc
    assert b'already' in e.f['last_error']()
    rep = e.alloc.torch.zeros(crs.report_words(4) + 2, dtype=e.alloc.torch.int64, device=e.alloc.device)
    table = np.zeros(eng.MAX_AGES, dtype=np.uint8)
    for n_days in (0, eng.MAX_DAYS + 1):
        assert f['course_report'](course._h, table.ctypes.data, 1, n_days, rep.data_ptr(), e.alloc.stream()) == -1
        assert b'n_days' in e.f['last_error']()
    assert f['course_report'](course._h, table.ctypes.data, 1, 4, rep.data_ptr() + 8, e.alloc.stream()) == -1
    assert b'aligned' in e.f['last_error']()
    assert f['course_report'](course._h, table.ctypes.data, 0, 4, rep.data_ptr(), e.alloc.stream()) == -1
    assert f['course_report'](course._h, table.ctypes.data, 1, 4, rep.data_ptr(), e.alloc.stream()) == 0
    out = np.zeros(e.config.n_agents, dtype=np.uint64)
    assert f['course_read'](course._h, 1, out.ctypes.data, e.alloc.stream()) == -1 and b'member' in e.f['last_error']()
    assert f['course_write'](course._h, 1, out.ctypes.data, e.alloc.stream()) == -1 and b'member' in e.f['last_error']()
    assert f['course_read'](course._h, 0, out.ctypes.data, e.alloc.stream()) == 0
    with pytest.raises(ValueError, match='transmission log'):
        c.snapshot()
    with pytest.raises(ValueError, match='already'):
        c.start_course_log()
    # the log goes first: the course refuses from then on, and goes without harm
    c.transmission_log.device.course = None
    c.transmission_log.device.close()
    assert f['course_read'](course._h, 0, out.ctypes.data, e.alloc.stream()) == -1 and b'gone' in e.f['last_error']()
    course.close()
