"""The detection report on the GPU: the device route (k_detect_report through reina_detect_report) against the numpy
specification of the read-back state -- hot words, cold words 2 and 3, log words, course records -- on simulated runs, on
synthetic states at tile edges and of every combination, on engine groups, on a logged particle filter, on a restored Context,
the refusals through the C ABI and the number of library calls each route makes.  The report is a function of the state, the
log and the course, so no host-driven reference run is needed.  Exact equality of words throughout.

Nothing here provokes anything: a synthetic state (detection_util) is NOT one a simulation could reach; it goes through a report
only and is never stepped."""
import collections
import copy
import gc

import numpy as np
import pytest

import course_util
import detection_util as du
import filter_util
import par_backend
import snap_util
import tx_util
import txlog_util as tu
from filter_util import small_scenario
from reina_model_amd import detection as det
from reina_model_amd import engine as eng
from reina_model_amd import ensemble, filtering, reports, simulation
from reina_model_amd.variables import VARIABLE_DEFAULTS

pytestmark = pytest.mark.gpu

DAYS = 120
FINE = np.minimum(np.arange(101) // 7, 15)   # a 16-group table


@pytest.fixture(autouse=True)
def _engines_go_with_their_test():
    """A logged Context and its log refer to each other: its engine goes only when the cycle collector runs"""
    yield
    gc.collect()


def _make(v, ages=None, seed=1, **kw):
    return simulation.make_context(v, age_counts=ages, seed=seed, ipc=None, **kw)


def _report_equals_spec(ctx, n_days=None, groups=None):
    assert ctx.course_log.on_device and ctx.course_log.device.group is None and ctx.engine.detect_f is not None
    got = ctx.course_log.detection_report(groups, n_days)
    du.assert_words(got.words, du.spec_report(ctx, n_days, groups).words)
    return got


# ---------------------------------------------------------------------------------------------- simulated runs

@pytest.mark.parametrize('env', ('REINA_DAY_MODE=dense', 'REINA_DAY_MODE=sparse', ''))
def test_tracing_120_days_device_report_equals_spec(env, monkeypatch):
    if env:
        monkeypatch.setenv(*env.split('='))
    v, ages = course_util.tracing_scenario()
    ctx = _make(v, ages, 3, course=True)
    ctx.run(DAYS)
    r = _report_equals_spec(ctx)
    assert r.n_days == DAYS and r.breach == r.out_of_range == r.before == r.bad_links == 0
    assert r.dated > 500 and r.never > 100 and r.linked > 1000 and int(r.phase[:, 0].sum()) > 0 and r.adjacent_share(1) > 0
    short = _report_equals_spec(ctx, n_days=50)              # (most known days out of range)
    assert short.out_of_range > 0
    _report_equals_spec(ctx, n_days=eng.MAX_DAYS)
    fine = _report_equals_spec(ctx, groups=FINE)
    assert fine.n_groups == 15 and fine.linked == r.linked
    _report_equals_spec(ctx, n_days=eng.MAX_DAYS, groups=FINE)


def test_hus_200_days_under_the_default_interventions():
    ctx = _make(copy.deepcopy(VARIABLE_DEFAULTS), None, 5, course=True)
    ctx.run(200)
    r = _report_equals_spec(ctx)
    assert r.breach == 0 and r.infected > 50000 and r.dated > 1000 and r.linked > 50000 and r.out_of_range == 0


# ---------------------------------------------------------------------------------------------- synthetic states

def _synthetic(hot, inf, cnt, log, rec):
    ctx = du.put_state(snap_util.make_context(len(hot)), hot, inf, cnt, log, rec)
    assert ctx.course_log.on_device
    got = du.host_arrays(ctx)
    assert np.array_equal(got[0], hot) and np.array_equal(got[1], inf) and np.array_equal(got[2], cnt)
    assert np.array_equal(ctx.transmission_log.words(), log) and np.array_equal(ctx.course_log.words(), rec)
    return ctx


def _synthetic_report(ctx, state, n_days, kind='default'):
    g = tx_util.groups(kind)
    got = ctx.course_log.detection_report(g, n_days)
    want = det.report_numpy(*state, np.asarray(ctx.engine.config.age_start), g, n_days)
    du.assert_words(got.words, want.words)
    return got


@pytest.mark.parametrize('n', tu.SIZES)
def test_report_kernel_equals_spec_at_tile_edges(n):
    state = du.forest_state(n)
    ctx = _synthetic(*state)
    r = _synthetic_report(ctx, state, du.N_DAYS, 'fine' if n % 2 else 'default')
    assert r.infected == int(((state[0] & 7) != 0).sum()) == r.roots + r.linked + r.bad_links
    if n > 500:
        assert r.bad_links > 0 and r.breach > 0
    _synthetic_report(ctx, state, 1)


def test_report_kernel_equals_spec_on_every_combination():
    state = du.combos_state()
    ctx = _synthetic(*state)
    r = _synthetic_report(ctx, state, du.N_DAYS)
    assert all(getattr(r, name) > 0 for name in det.SCALAR_NAMES) and (r.link_class.sum(axis=0) > 0).all() and (r.phase.sum(axis=0) > 0).all()
    _synthetic_report(ctx, state, 1)
    _synthetic_report(ctx, state, eng.MAX_DAYS, 'fine')


@pytest.mark.parametrize('which', ('even_tiles_empty', 'every_agent_a_root'))
def test_the_tile_skip_and_the_gathers_not_taken(which):
    n = tu.SIZES[-1]
    hot, inf, cnt, log, rec = du.forest_state(n, seed=2)
    if which == 'even_tiles_empty':            # both sides of the tile skip; the links into the emptied tiles turn bad
        hot = np.where((np.arange(n) // 512) % 2 == 0, 0, hot).astype(np.uint32)
    else:                                      # no infector: no gather of an infector's words or record is taken
        inf = np.full(n, -1, dtype=np.int32)
    state = (hot, inf, cnt, log, rec)
    ctx = _synthetic(*state)
    r = _synthetic_report(ctx, state, du.N_DAYS)
    if which == 'even_tiles_empty':
        assert 100 < r.infected == int(((hot & 7) != 0).sum()) and r.bad_links > 50 and r.linked > 50
    else:
        assert r.roots == r.infected > 100 and r.linked == 0 and not r.link_class.any() and not r.pair_class.any()
    _synthetic_report(ctx, state, 1)


# ---------------------------------------------------------------------------------------------- groups, filters, snapshots

@pytest.mark.parametrize('members', (1, 3, 4))
def test_logged_groups_equal_single_contexts(members):
    v, ages = course_util.tracing_scenario()
    seeds, days = list(range(40, 40 + members)), 60
    planner = _make(v, ages, seeds[0])
    ctxs = [_make(v, ages, sd) for sd in seeds]
    ensemble.run_group_plan(ctxs, planner.make_plan(days), course=True)
    glog = ctxs[0].transmission_log.device
    assert glog.group is not None and glog.course is not None and all(c.course_log.device is glog.course for c in ctxs)
    reps = ensemble.detection_reports(ctxs)
    assert len(reps) == members
    for m, sd in enumerate(seeds):
        du.assert_words(reps[m].words, du.spec_report(ctxs[m]).words)
        du.assert_words(reps[m].words, ctxs[m].course_log.detection_report().words)   # (a member's own report: the numpy route)
        solo = _make(v, ages, sd, course=True)
        solo.run(days)
        du.assert_words(reps[m].words, _report_equals_spec(solo).words)
        del solo
        assert reps[m].n_days == days and reps[m].dated > 0 and reps[m].breach == 0
    assert all(not np.array_equal(reps[0].words, r.words) for r in reps[1:]), 'the members differ by seed'
    fine = ensemble.detection_reports(ctxs, age_groups=FINE, n_days=30)
    for m in range(members):
        du.assert_words(fine[m].words, du.spec_report(ctxs[m], 30, FINE).words)
    for c in ctxs:
        c.transmission_log = c.course_log = None
    glog.close()
    glog.group.close()


def test_logged_filter_reports_every_final_particle():
    K, days, window = 4, 21, 7
    v, ages = course_util.tracing_scenario()
    truth = simulation.make_context(v, age_counts=ages, seed=777, ipc='auto', engine_factory=par_backend.par_engine_factory)
    obs = filter_util.observations(truth.run(days), v['start_date'], range(1, days))
    model = filtering.ObservationModel({'all_detected': 8.0, 'in_ward': 8.0})
    r = filtering.particle_filter(v, K, observations=obs, obs_model=model, window=window, days=days, ess_threshold=1.0,
                                  seeds=list(range(100, 100 + K)), filter_seed=5, age_counts=ages, course=True)
    try:
        assert len(r.windows) == 3 and r.log is not None and r.log.course is not None
        reps = r.detection_reports()
        assert len(reps) == K
        for k, c in enumerate(r.contexts):
            want = du.spec_report(c, days, log_words=r.log.words(k), records=r.log.course.words(k))
            du.assert_words(reps[k].words, want.words)
            assert reps[k].n_days == days and reps[k].infected > 0 and reps[k].breach == 0
    finally:
        r.close()
    with pytest.raises(ValueError, match='closed'):
        r.detection_reports()


def test_restored_context_with_a_course_begun_at_day_120():
    v, ages = course_util.tracing_scenario()
    b = _make(v, ages, 3)
    b.run(120)
    c = _make(v, ages, 3, snapshot=b.snapshot(), course=True)
    assert c.day == 120 and c.course_log.begin_day == 120 and c.course_log.on_device
    c.run(40)
    r = _report_equals_spec(c)
    assert r.before > 0 and int(r.link_class[:, 4].sum()) > 0 and r.breach == 0 and int(r.detections[:120].sum()) == 0


# ---------------------------------------------------------------------------------------------- refusals

def test_refusals_through_the_c_abi():
    v, ages = course_util.tracing_scenario()
    c = _make(v, ages, 1, course=True)
    c.run(20)
    e, course = c.engine, c.course_log.device
    f, stream, torch = e.detect_f, e.alloc.stream(), e.alloc.torch
    UNTOUCHED = -77
    rep = torch.full((det.report_words(4) + 2,), UNTOUCHED, dtype=torch.int64, device=e.alloc.device)
    table = np.zeros(eng.MAX_AGES, dtype=np.uint8)
    high = table.copy()
    high[5] = 3
    last = lambda: e.f['last_error']()
    for n_days in (0, eng.MAX_DAYS + 1):
        assert f['detect_report'](course._h, table.ctypes.data, 1, n_days, rep.data_ptr(), stream) == -1
        assert b'detection report: n_days must be in [1, REINA_MAX_DAYS]' in last()
    assert f['detect_report'](course._h, high.ctypes.data, 3, 4, rep.data_ptr(), stream) == -1
    assert b"detection report: an age's group is not below n_groups" in last()
    assert f['detect_report'](course._h, table.ctypes.data, 0, 4, rep.data_ptr(), stream) == -1 and b'n_groups' in last()
    assert f['detect_report'](course._h, table.ctypes.data, det.MAX_GROUPS + 1, 4, rep.data_ptr(), stream) == -1 and b'n_groups' in last()
    assert f['detect_report'](course._h, None, 1, 4, rep.data_ptr(), stream) == -1
    assert f['detect_report'](course._h, table.ctypes.data, 1, 4, rep.data_ptr() + 8, stream) == -1
    assert b'detection report: the report must be a 16-byte aligned device buffer' in last()
    assert f['detect_report'](course._h, table.ctypes.data, 1, 4, None, stream) == -1 and b'aligned' in last()
    assert f['detect_report'](None, table.ctypes.data, 1, 4, rep.data_ptr(), stream) == -1
    torch.cuda.synchronize()
    assert bool((rep == UNTOUCHED).all()), 'a refused call queued something'
    assert f['detect_report'](course._h, table.ctypes.data, 1, 4, rep.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    got = rep.cpu().numpy()
    want = du.spec_report(c, 4, np.zeros(101, dtype=np.int64))
    du.assert_words(got[:det.report_words(4)].view(np.uint64), want.words)
    assert (got[det.report_words(4):] == UNTOUCHED).all(), 'the block is report_words(n_days) words'
    # the log goes first: the course refuses from then on
    rep.fill_(UNTOUCHED)
    c.transmission_log.device.course = None
    c.transmission_log.device.close()
    assert f['detect_report'](course._h, table.ctypes.data, 1, 4, rep.data_ptr(), stream) == -1 and b'gone' in last()
    torch.cuda.synchronize()
    assert bool((rep == UNTOUCHED).all()), 'a refused call queued something'
    course.close()


# ---------------------------------------------------------------------------------------------- route counts

@pytest.fixture
def calls(monkeypatch):
    """{entry-point name: calls} of reports.device_words from here on (tests/test_report_routes_gpu.py)"""
    seen = collections.Counter()
    inner = reports.device_words

    def counting(engine, f, name, *args, **kw):
        seen[name] += 1
        return inner(engine, f, name, *args, **kw)

    monkeypatch.setattr(reports, 'device_words', counting)
    return seen


def _small(seed, **kw):
    v, ages = small_scenario(700)
    return simulation.make_context(v, age_counts=ages, seed=seed, ipc='auto', **kw)


def test_a_whole_group_is_one_call_a_member_alone_is_none_and_other_reports_call_nothing_new(calls):
    planner = _small(11)
    ctxs = [_small(11 + m) for m in range(4)]
    ensemble.run_group_plan(ctxs, planner.make_plan(12), course=True)
    glog = ctxs[0].transmission_log.device
    try:
        assert not calls, 'a run without a detection report issues no report call'
        whole = ensemble.detection_reports(ctxs)
        assert dict(calls) == {'detect_report': 1} and len(whole) == 4
        calls.clear()
        alone = ctxs[2].course_log.detection_report()
        part = ensemble.detection_reports([ctxs[0], ctxs[2]])
        assert dict(calls) == {}, 'a member taken alone takes the numpy route'
        assert alone == whole[2] and part == [whole[0], whole[2]]
        ensemble.course_reports(ctxs), ensemble.log_reports(ctxs), ensemble.vaccination_reports(ctxs)
        assert dict(calls) == {'course_report': 1, 'group_txlog_report': 1, 'vacc_report': 1}, 'the other reports call what they called'
    finally:
        for c in ctxs:
            c.transmission_log = c.course_log = None
        group = glog.group
        glog.close()
        group.close()
    calls.clear()
    c = _small(5, course=True)
    c.run(12)
    assert not calls
    one = c.course_log.detection_report()
    assert dict(calls) == {'detect_report': 1} and ensemble.detection_reports([c]) == [one] and dict(calls) == {'detect_report': 2}
    c.course_log.close()
    c.transmission_log.close()
