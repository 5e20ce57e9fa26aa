"""Logged particle filters on the GPU (include/reina_filter_log.h): reina_group_txlog_clone against the dense copy on simulated
groups at tile edges, a cloned member with its logs continued against a restored snapshot under both forms of k_txlog_day,
the refusals through the C ABI, a whole logged filter -- every final particle's reports against the numpy specification and
against the counters along its ancestral path --, and the unlogged filter, which the logs leave as it was.  Exact equality
throughout."""
import ctypes
import gc

import numpy as np
import pytest

import filter_util
import par_backend
import txlog_util as tu
from filter_log_util import CLONE_DAY, classes, incidence_by_day
from filter_util import assert_same_day_state, small_scenario, totals
from reina_model_amd import course as crs
from reina_model_amd import engine as eng
from reina_model_amd import ensemble, filtering, simulation

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _engines_go_with_their_test():
    """A logged Context and its log refer to each other, so its engine goes only when the cycle collector runs.  The library
    counts its live engines (who may take the one-launch day, tests/test_parity_gpu.py): none of this module's stay behind."""
    yield
    gc.collect()


def _release(ctxs, glog, group):
    for c in ctxs:
        c.transmission_log = c.course_log = None
    glog.close()
    group.close()


def _make(v, ages, seed, **kw):
    return simulation.make_context(v, age_counts=ages, seed=seed, ipc='auto', **kw)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    bad = np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1)) if got.ndim else np.flatnonzero(got != want)
    assert len(bad) == 0, '%s: %d rows differ, first %d' % (what, len(bad), bad[0])


def _logged_group(n, seeds, days, course):
    """K Contexts of small_scenario(n) run `days` days as one logged group: (v, ages, planner, contexts, device log, group)"""
    v, ages = small_scenario(n)
    planner = _make(v, ages, seeds[0])
    ctxs = [_make(v, ages, sd) for sd in seeds]
    ensemble.run_group_plan(ctxs, planner.make_plan(days), txlog=True, course=course)
    glog = ctxs[0].transmission_log.device
    assert glog is not None and glog.group is not None and (glog.course is not None) == course
    return v, ages, planner, ctxs, glog, glog.group


def _everything(ctxs, glog):
    """per member: the carried arrays, the log words and the course records (host copies)"""
    out = []
    for m, c in enumerate(ctxs):
        d = filter_util.carried(c.engine)
        d['log'] = glog.words(m)
        if glog.course is not None:
            d['records'] = glog.course.words(m)
        out.append(d)
    return out


def _assert_untouched(ctxs, glog, before, members, what):
    after = _everything(ctxs, glog)
    for m in members:
        for name, w in before[m].items():
            _same(after[m][name], w, '%s: member %d %s' % (what, m, name))


# ---------------------------------------------------------------------------------------------- 1. the clone, directly

@pytest.mark.parametrize('course', (True, False), ids=('course', 'log-only'))
@pytest.mark.parametrize('pairs', ([(1, 0), (3, 2)], [(1, 0), (3, 0)]), ids=('two-sources', 'shared-source'))
@pytest.mark.parametrize('n', (20000, 20480, 700))   # a ragged last tile, whole tiles, two tiles
def test_clone_carries_the_logs(n, pairs, course):
    v, ages, planner, ctxs, glog, group = _logged_group(n, [11, 12, 13, 14], CLONE_DAY, course)
    try:
        before = _everything(ctxs, glog)
        if n == 20000:
            for d, s in pairs:
                assert min(classes(before[d]['hot'], before[s]['hot'])) > 0, 'recorded in both, in src only, in dst only, in neither'
        for d, s in pairs:
            assert not np.array_equal(before[d]['log'], before[s]['log'])
        filtering.clone_group(group, pairs, log=glog)
        after = _everything(ctxs, glog)
        for d, s in pairs:
            _same(after[d]['log'], before[s]['log'], 'member %d <- %d: log words' % (d, s))
            if course:
                _same(after[d]['records'], before[s]['records'], 'member %d <- %d: records' % (d, s))
            _same(after[d]['hot'], before[s]['hot'], 'member %d <- %d: hot words' % (d, s))
            assert_same_day_state(ctxs[d], ctxs[s])
        dsts = [d for d, _ in pairs]
        _assert_untouched(ctxs, glog, before, [m for m in range(len(ctxs)) if m not in dsts], 'after the clone')
    finally:
        _release(ctxs, glog, group)


# ---------------------------------------------------------------------------------------------- 2. continuation

@pytest.mark.parametrize('course', (True, False), ids=('course', 'log-only'))
@pytest.mark.parametrize('form', ('', 'log'), ids=('hot-word-form', 'log-word-form'))
def test_cloned_member_with_its_logs_continues_like_a_restored_snapshot(form, course, monkeypatch):
    """a group of three runs to `cut`; member a is cloned into member m, logs and all; the group runs `days` more.  Reference:
    a fresh Context of m's seed restored from a snapshot of an unlogged run of a's seed at `cut`, its logs begun there and
    their words set to a's saved ones."""
    if form:
        monkeypatch.setenv('REINA_TXLOG_FORM', form)
    seeds, a, m, cut, days = [41, 42, 43], 1, 0, 120, 30
    v, ages, planner, ctxs, glog, group = _logged_group(20000, seeds, cut, course)
    try:
        words_a = glog.words(a)
        rec_a = glog.course.words(a) if course else None
        filtering.clone_group(group, [(m, a)], log=glog)
        hist = ensemble.run_group_plan(ctxs, planner.make_plan(days))   # (the logs continue)
        solo = _make(v, ages, seeds[a])
        solo.run(cut)
        ref = _make(v, ages, seeds[m], snapshot=solo.snapshot(), txlog=True, course=course)
        assert ref.transmission_log.on_device and ref.transmission_log.begin_day == cut
        ref.transmission_log.set_words(words_a)
        if course:
            ref.course_log.set_words(rec_a)
        want = ref.run(days)
        _same(hist[m], want, 'history')
        _same(glog.words(m), ref.transmission_log.words(), 'log words')
        assert not np.array_equal(glog.words(m), words_a), 'the days after the clone were recorded'
        assert_same_day_state(ctxs[m], ref)
        lr = ensemble.log_reports(ctxs)[m]
        tu.assert_words(lr.words, ref.transmission_log.report().words)
        assert lr.before == 0 and lr.dated == lr.infected > 0 and lr.last_day == cut + days - 1
        if course:
            _same(glog.course.words(m), ref.course_log.words(), 'records')
            tu.assert_words(ensemble.course_reports(ctxs)[m].words, ref.course_log.report().words)
    finally:
        _release(ctxs, glog, group)


# ---------------------------------------------------------------------------------------------- 3. refusals through the C ABI

def test_refusals_leave_state_and_logs_untouched():
    v, ages, planner, ctxs, glog, group = _logged_group(700, [21, 22, 23, 24], 30, True)
    solo = _make(v, ages, 25, course=True)
    try:
        e = ctxs[0].engine
        f = e.filter_log_f
        assert f is not None and f['filter_log_version']() == 1
        before = _everything(ctxs, glog)

        def call(handle, pairs):
            flat = [x for pr in pairs for x in pr]
            arr = (ctypes.c_uint32 * max(len(flat), 1))(*flat)
            return f['group_txlog_clone'](handle, arr, len(pairs), e.alloc.stream())

        for pairs, why in (([(1, 0), (1, 2)], b'a destination appears twice'), ([(1, 0), (0, 2)], b'a source is also a destination'),
                           ([(2, 2)], b'a source is also a destination'), ([(4, 0)], b'out of range'), ([(1, 0), (2, 70000)], b'out of range')):
            assert call(glog._h, pairs) == -1
            assert why in e.f['last_error'](), (pairs, e.f['last_error']())
            assert b'reina_group_txlog_clone' in e.f['last_error']()
        assert call(solo.transmission_log.device._h, [(0, 0)]) == -1 and b'made for one engine' in e.f['last_error']()
        assert call(None, [(1, 0)]) == -1 and b'no log' in e.f['last_error']()
        assert f['group_txlog_clone'](glog._h, None, 1, e.alloc.stream()) == -1 and b'no pair list' in e.f['last_error']()
        with pytest.raises(eng.EngineError):
            filtering.clone_group(group, [(1, 0), (1, 2)], log=glog)
        with pytest.raises(ValueError, match='not the transmission log of this group'):
            filtering.clone_group(group, [(1, 0)], log=solo.transmission_log.device)
        assert call(glog._h, []) == 0            # (nothing to do)
        filtering.clone_group(group, [], log=glog)
        e.alloc.torch.cuda.synchronize()
        _assert_untouched(ctxs, glog, before, range(len(ctxs)), 'after the refused calls')
        # the unlogged entry point keeps its messages
        with pytest.raises(eng.EngineError):
            filtering.clone_group(group, [(1, 0), (1, 2)])
        assert b'reina_group_clone: a destination appears twice' in e.f['last_error']()
    finally:
        _release(ctxs, glog, group)


# ---------------------------------------------------------------------------------------------- 4. the filter

K, DAYS, WINDOW = 8, 56, 7
Q = (0.05, 0.5, 0.95)


def _filter(**kw):
    v, ages = small_scenario(20000)
    truth = simulation.make_context(v, age_counts=ages, seed=777, ipc='auto', engine_factory=par_backend.par_engine_factory)
    obs = filter_util.observations(truth.run(DAYS), v['start_date'], range(1, DAYS))
    model = filtering.ObservationModel({'all_detected': 8.0, 'in_ward': 8.0})
    return filtering.particle_filter(v, K, observations=obs, obs_model=model, window=WINDOW, days=DAYS, ess_threshold=1.0,
                                     seeds=list(range(100, 100 + K)), filter_seed=5, age_counts=ages, **kw)


@pytest.fixture(scope='module')
def logged():
    """the logged filter, and what it held when it returned (the forecast of the test below extends it)"""
    r = _filter(txlog=True, course=True)
    kept = dict(paths=r.paths().copy(), ancestors=r.ancestors.copy(), loglik=r.loglik.copy(), log_evidence=r.log_evidence,
                finals=[np.asarray(c.engine.read_counters()).copy() for c in r.contexts])
    yield r, kept
    r.close()
    del r, kept
    gc.collect()


def _assert_incidence_follows_the_paths(r, reports):
    paths = r.paths()
    for k, rep in enumerate(reports):
        rows = np.concatenate([paths[k], np.asarray(r.contexts[k].engine.read_counters())[None]])
        inc = incidence_by_day(rep)
        assert len(inc) == paths.shape[1]
        bad = np.flatnonzero(inc != np.diff(totals(rows, 'all_infected')))
        assert len(bad) == 0, 'particle %d: the incidence of day %d is not the increment along its path' % (k, bad[0])


def test_logged_filter_reports_every_particles_whole_path(logged):
    r, kept = logged
    assert len(r.windows) == DAYS // WINDOW and sum(w['resampled'] for w in r.windows) >= 5, 'ess_threshold = 1: the windows resample'
    assert any(not np.array_equal(w['ancestors'], np.arange(K)) for w in r.windows), 'the logs had to travel'
    moved = sum(int((w['ancestors'] != np.arange(K)).sum()) for w in r.windows)
    glog = r.log
    assert glog is not None and glog.course is not None and glog.group is r.group
    reports, creports = r.log_reports(), r.course_reports()
    assert len(reports) == len(creports) == K
    for k, c in enumerate(r.contexts):
        hot, inf, cnt = tu.host_state(c)
        table = c._tx_groups(None)[0]
        words, rec = glog.words(k), glog.course.words(k)
        tu.assert_words(reports[k].words, tu.spec_report(c, words, DAYS).words)
        tu.assert_words(creports[k].words, crs.report_numpy(hot, words, rec, c.age_start, table, DAYS).words)
        assert reports[k].before == 0 and reports[k].dated == reports[k].infected > 0 and reports[k].n_days == DAYS
    # ... which holds only if the logs travelled with the ancestors
    _assert_incidence_follows_the_paths(r, reports)
    lin = r.lineage_reports()
    assert len(lin) == K
    # the bands are weighted_band over the per-particle reports
    frames = [rep.case_reproduction_number() for rep in reports]
    band = r.reproduction_number_band(Q)
    assert list(band.columns) == list(Q) + ['cohort', 'closed_share'] and len(band) == DAYS and band.index.equals(frames[0].index)
    rc = np.stack([f['r_c'].to_numpy() for f in frames])
    assert np.array_equal(band[list(Q)].to_numpy(), r.weighted_band(rc, Q), equal_nan=True)
    assert np.isfinite(band[0.5].to_numpy()).sum() > DAYS // 2
    w = r.weights
    np.testing.assert_allclose(band['cohort'].to_numpy(), (np.stack([f['cohort'].to_numpy() for f in frames]) * w[:, None]).sum(axis=0), rtol=1e-12)
    adm = np.stack([rep.admissions.sum(axis=1).astype(np.float64) for rep in creports])
    assert np.array_equal(r.admissions_band(Q).to_numpy(), r.weighted_band(adm, Q)) and adm.sum() > 0
    inc = np.stack([incidence_by_day(rep).astype(np.float64) for rep in reports])
    assert np.array_equal(r.incidence_band(Q).to_numpy(), r.weighted_band(inc, Q))
    print('logged filter: %d members moved over %d windows; median R_c on day 20: %.2f' % (moved, len(r.windows), band[0.5].iloc[20]))
    # a forecast continues the logs
    r.forecast(7)
    longer = r.log_reports()
    assert all(rep.n_days == DAYS + 7 for rep in longer) and max(rep.last_day for rep in longer) >= DAYS
    for k in range(K):
        assert np.array_equal(longer[k].incidence[:DAYS], reports[k].incidence)
    _assert_incidence_follows_the_paths(r, longer)
    assert len(r.admissions_band(Q)) == DAYS + 7


def test_a_logged_filter_from_a_snapshot_marks_the_past_before():
    v, ages = small_scenario(20000)
    cut, days = 40, 14
    solo = _make(v, ages, 9)
    solo.run(cut)
    infected = int(np.count_nonzero(tu.host_state(solo)[0] & 7))
    r = filtering.particle_filter(v, 4, None, days=days, window=7, seeds=[1, 2, 3, 4], age_counts=ages, snapshot=solo.snapshot(), txlog=True)
    try:
        assert r.log is not None and r.log.course is None and infected > 100
        paths = r.paths()
        for k, rep in enumerate(r.log_reports()):
            assert rep.n_days == cut + days and rep.before == infected and rep.dated == rep.infected - infected > 0
            assert rep.first_day >= cut
            inc = incidence_by_day(rep)
            rows = np.concatenate([paths[k], np.asarray(r.contexts[k].engine.read_counters())[None]])
            assert inc[:cut].sum() == 0 and np.array_equal(inc[cut:], np.diff(totals(rows, 'all_infected')))
        with pytest.raises(ValueError, match='keeps no course log'):
            r.admissions_band()
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------- 5. the logs observe, never steer

def test_unlogged_filter_is_unchanged(logged):
    _, kept = logged
    r = _filter()
    try:
        assert r.log is None and all(c.transmission_log is None for c in r.contexts)
        assert np.array_equal(r.ancestors, kept['ancestors'])
        assert np.array_equal(r.loglik, kept['loglik']) and r.log_evidence == kept['log_evidence']
        assert np.array_equal(r.paths(), kept['paths'])
        for c, final in zip(r.contexts, kept['finals']):
            assert np.array_equal(np.asarray(c.engine.read_counters()), final)
        with pytest.raises(ValueError, match='keeps no transmission log'):
            r.reproduction_number_band()
    finally:
        r.close()
