"""The clinical course log on the CPU: the numpy specification (reina_model_amd/course.py) against a plain per-agent walker on
synthetic states, begin and record on hand-made hot words, simulated runs on oracle B through run_host_driven -- with the
property k_course_day relies on (the ACTIVE agents are enough) held day by day --, conservation against the engine's own
counters, the header against the module, and the refusals.  Every comparison is of integers and exact."""
import os
import re

import numpy as np
import pytest

import course_util as cu
import par_backend
import tx_util
from filter_util import small_scenario, totals
from reina_model_amd import course as crs
from reina_model_amd import engine as eng
from reina_model_amd import simulation, txlog as txl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, B = txl.NONE, txl.BEFORE
R = lambda det, adm, icu, out: int(crs.pack([det], [adm], [icu], [out])[0])


# ---------------------------------------------------------------------------------------------- 1. report_numpy == walker

def _spec_and_walk(hot, log, rec, n_days=cu.N_DAYS, kind='default'):
    n = len(hot)
    age_start, g = tx_util.age_start_of(n), tx_util.groups(kind)
    r = crs.report_numpy(hot, log, rec, age_start, g, n_days)
    cu.assert_words(r.words, cu.walk_report(hot, log, rec, age_start, [int(x) for x in g], n_days))
    return r


@pytest.mark.parametrize('n', (1, 511, 512, 513, 3 * 512 + 7))
def test_spec_equals_walker_on_random_records(n):
    hot, _, _, log, rec = cu.forest_state(n)
    _spec_and_walk(hot, log, rec, kind='fine' if n % 2 else 'default')


def test_spec_equals_walker_on_every_code_combination_and_clipping():
    hot, _, _, log, rec = cu.combos_state()
    r = _spec_and_walk(hot, log, rec)
    assert (r.pathway.sum(axis=0) > 0).all(), 'every pathway class occurs'
    assert (r.delay_n.sum(axis=1) > 0).all(), 'every delay kind occurs'
    for k in range(crs.KINDS):   # both end bins of every histogram are hit
        h = r.delay_counts[k].sum(axis=0)
        assert h[0] >= 2 and h[-1] >= 2, k
    assert r.out_of_range > 0 and r.detected_undated > 0 and r.died_outside > 0
    assert int(r.delay_sum.min()) < 0 or int(r.delay_counts[:, :, 0].sum()) > 0
    _spec_and_walk(hot, log, rec, n_days=1)
    _spec_and_walk(hot, log, rec, n_days=eng.MAX_DAYS, kind='fine')


def test_report_accessors():
    hot, _, _, log, rec = cu.combos_state()
    r = _spec_and_walk(hot, log, rec)
    for name in ('admissions', 'detections', 'deaths'):
        f = getattr(r, name + '_frame')()
        assert f.shape == (cu.N_DAYS, r.n_groups) and int(f.values.sum()) == int(getattr(r, name).sum())
    d = r.delay('onset_to_admission')
    assert d.total() == int(r.delay_n[1].sum()) and d.mean() == int(r.delay_sum[1].sum()) / d.total()
    assert d.series().index[0] == 0 and d.quantile(0.5) is not None
    d0 = r.delay('onset_to_detection')
    assert d0.series().index[0] == -16 and d0.mean() == int(r.delay_sum[0].sum()) / d0.total() - 16
    assert r.length_of_stay('ward', 'dead').total() == int(r.delay_n[4].sum())
    assert r.length_of_stay('icu', 'recovered').total() == int(r.delay_n[5].sum())
    with pytest.raises(ValueError):
        r.length_of_stay('home', 'dead')
    p = r.pathways_frame()
    assert list(p.columns) == list(crs.CLASS_NAMES) and int(p.values.sum()) == r.infected
    for f, field in ((r.fatality_by_cohort(), 3), (r.hospitalisation_by_cohort(), 2)):
        assert list(f.columns)[1:] == ['cohort', 'closed_share'] and int(f['cohort'].sum()) == int(r.cohort[..., 0].sum())
        day = int(np.flatnonzero(r.cohort[..., 0].sum(axis=1))[0])
        assert f.iloc[day, 0] == r.cohort[day, :, field].sum() / r.cohort[day, :, 0].sum()
    empty = crs.report_numpy(np.zeros(600, dtype=np.uint32), np.zeros(600, dtype=np.uint32), np.zeros(600, dtype=np.uint64),
                             tx_util.age_start_of(600), tx_util.groups(), 10)
    assert empty.infected == 0 and not empty.words.any() and empty.delay('onset_to_death').mean() is None


# ---------------------------------------------------------------------------------------------- 2. begin and record

def test_begin_and_record_on_hand_made_hot_words():
    S = lambda st, det=0: np.uint32(st | det | 0x8000)
    D = cu.DETECTED
    hot = np.array([0, D, S(1), S(1, D), S(2), S(2, D), S(3), S(3, D), S(4), S(4, D), S(5), S(6, D)], dtype=np.uint32)
    rec = crs.begin_numpy(hot)
    assert [int(x) for x in rec] == [R(N, N, N, N), R(N, N, N, N), R(N, N, N, N), R(B, N, N, N), R(N, N, N, N), R(B, N, N, N),
                                    R(N, B, N, N), R(B, B, N, N), R(N, B, B, N), R(B, B, B, N), R(B, B, B, B), R(B, B, B, B)]
    assert rec.dtype == np.uint64
    assert np.array_equal(crs.record_numpy(rec, hot, 7), rec), 'BEFORE is never overwritten, and nothing new has happened'
    # every transition from NONE
    rec = np.full(len(hot), R(N, N, N, N), dtype=np.uint64)
    got = crs.record_numpy(rec, hot, 9)
    assert [int(x) for x in got] == [R(N, N, N, N), R(N, N, N, N), R(N, N, N, N), R(9, N, N, N), R(N, N, N, N), R(9, N, N, N),
                                    R(N, 9, N, N), R(9, 9, N, N), R(N, 9, 9, N), R(9, 9, 9, N), R(N, N, N, 9), R(9, N, N, 9)]
    # ward on day 9, ICU on day 12, dead on day 20; a detection on day 25 comes too late
    one = np.array([R(N, 9, N, N)], dtype=np.uint64)
    one = crs.record_numpy(one, np.array([S(4)]), 12)
    assert int(one[0]) == R(N, 9, 12, N)
    one = crs.record_numpy(one, np.array([S(6)]), 20)
    assert int(one[0]) == R(N, 9, 12, 20)
    assert int(crs.record_numpy(one, np.array([S(6, D)]), 25)[0]) == R(N, 9, 12, 20), 'a record closes with its outcome'
    # `where`: an agent outside the mask keeps its record
    two = crs.record_numpy(np.full(2, R(N, N, N, N), dtype=np.uint64), np.array([S(3), S(3)]), 4, where=[True, False])
    assert [int(x) for x in two] == [R(N, 4, N, N), R(N, N, N, N)]
    with pytest.raises(ValueError):
        crs.record_numpy(one, hot[:1], eng.MAX_DAYS)
    assert all(int(a[0]) == b for a, b in zip(crs.fields(np.array([R(1, 2, 3, 4)], dtype=np.uint64)), (1, 2, 3, 4)))


# ---------------------------------------------------------------------------------------------- 3. simulated runs on oracle B

def _oracle(v, ages, seed, ipc='auto', **kw):
    return simulation.make_context(v, age_counts=ages, seed=seed, ipc=ipc, engine_factory=par_backend.par_engine_factory, **kw)


class ActiveFacts:
    """run_host_driven's on_day handle: after every day, record_numpy restricted to the agents with RH_ACTIVE set equals
    record_numpy over all agents -- what lets k_course_day stream the ACTIVE plane alone"""

    def __init__(self):
        self.changed = 0
        self.hot_at = {}
        self.keep = ()

    def __call__(self, day, hot, before, after):
        active = (hot & cu.ACTIVE) != 0
        assert np.array_equal(crs.record_numpy(before, hot, day, where=active), after), 'day %d: an agent that is not ACTIVE changed its record' % day
        ch = before != after
        assert active[ch].all(), day
        st = hot[ch] & 7
        assert (st >= 2).all() or ((hot[ch] & cu.DETECTED) != 0)[st < 2].all(), 'day %d: a record of an undetected incubating agent changed' % day
        self.changed += int(ch.sum())
        if day + 1 in self.keep:
            self.hot_at[day + 1] = hot.copy()


def _run(v, ages, seed, days, ipc='auto', keep=()):
    ctx = _oracle(v, ages, seed, ipc)
    facts = ActiveFacts()
    facts.keep = keep
    hist = crs.run_host_driven(ctx, days, on_day=facts)
    assert ctx.course_log is not None and not ctx.course_log.on_device and facts.changed > 0
    return ctx, hist, facts


@pytest.fixture(scope='module')
def mini_200():
    v, ages = small_scenario()
    return _run(v, ages, 3, 200, keep=(60,))


@pytest.fixture(scope='module')
def traced_200():
    v, ages = cu.tracing_scenario()
    return _run(v, ages, 3, 200)


def _report_equals_spec(ctx, n_days=None):
    r = ctx.course_log.report(n_days=n_days)
    hot = np.array(ctx.engine.tensors['hot']).view(np.uint32)
    want = crs.report_numpy(hot, ctx.transmission_log.words(), ctx.course_log.words(), ctx.age_start, ctx._tx_groups(None)[0],
                            max(ctx.day, 1) if n_days is None else n_days)
    assert r == want
    return r


def test_active_agents_are_enough_on_the_mini_population(mini_200):
    ctx, hist, facts = mini_200
    r = _report_equals_spec(ctx)
    assert r.with_admission > 50 and r.with_icu > 5 and r.with_outcome > 5000 and r.out_of_range == 0
    assert (r.pathway.sum(axis=0)[[3, 4, 5, 6]] > 0).all(), 'recoveries at home, from ward and from ICU, and deaths without a bed (care saturates)'
    assert int(r.pathway[:, 9].sum()) == 0, 'nothing is BEFORE in a course begun on day 0 without an initial condition'
    _report_equals_spec(ctx, n_days=50)


def test_active_agents_are_enough_with_an_initial_condition():
    v, ages = small_scenario()
    ctx, hist, facts = _run(v, ages, 5, 120, ipc=cu.IPC)
    r = _report_equals_spec(ctx)
    assert int(r.pathway[:, 9].sum()) >= cu.IPC['dead'] + cu.IPC['recovered'] + cu.IPC['in_icu'] + cu.IPC['in_ward']
    det, adm, icu, out = ctx.course_log.days()
    assert int((out == -2).sum()) >= cu.IPC['dead'] + cu.IPC['recovered'] and int((icu == -2).sum()) >= cu.IPC['in_icu']


def test_active_agents_are_enough_under_contact_tracing_and_late_detections_are_counted(traced_200):
    ctx, hist, facts = traced_200
    hot = np.array(ctx.engine.tensors['hot']).view(np.uint32)
    assert (hot & 0x4000).any(), 'contact tracing ran'
    r = _report_equals_spec(ctx)
    assert r.detected_undated > 0, 'tracing reaches agents whose record has closed'
    det, adm, icu, out = ctx.course_log.days()
    late = ((hot & cu.DETECTED) != 0) & ((hot & 7) != 0) & (det == -1)
    assert int(late.sum()) == r.detected_undated and ((hot[late] & 7) >= 5).all() and (out[late] >= 0).all()
    assert int(r.delay_counts[0, :, :crs.DETECTION_SHIFT].sum()) > 0, 'tracing detects before onset'


def test_conservation_against_the_engines_counters(mini_200, traced_200):
    """The counters by age, summed over the report's age groups.  REINA_C_DEAD, REINA_C_RECOVERED and REINA_C_CUM_ICU are
    cumulative: they equal the deaths, recoveries and agents with an ICU day.  REINA_C_HOSPITALIZED is an OCCUPANCY (an
    admission adds one, a release takes it back: DESIGN.md section 6k), so it equals the open records with an admission day,
    and the agents with an admission day are those plus the closed ones that had been admitted."""
    for ctx, hist, facts in (mini_200, traced_200):
        r = ctx.course_log.report()
        final = np.asarray(ctx.engine.read_counters())
        table = np.asarray(ctx._tx_groups(None)[0])[:ctx.nr_ages]

        def by_group(name):
            ci = eng.C_NAMES.index(name)
            c = final[ci * eng.MAX_AGES:ci * eng.MAX_AGES + ctx.nr_ages].astype(np.int64)
            return np.bincount(table, weights=c, minlength=crs.MAX_GROUPS).astype(np.int64)

        i64 = lambda a: np.asarray(a).astype(np.int64)
        assert np.array_equal(i64(r.deaths.sum(axis=0)), by_group('dead'))
        assert np.array_equal(i64(r.pathway[:, 6:9].sum(axis=1)), by_group('dead'))
        assert np.array_equal(i64(r.recoveries.sum(axis=0)), by_group('recovered'))
        assert np.array_equal(i64(r.icu_admissions.sum(axis=0)), by_group('cum_icu'))
        assert np.array_equal(i64(r.pathway[:, [2, 5, 8]].sum(axis=1)), by_group('cum_icu'))
        assert np.array_equal(i64(r.pathway[:, 1:3].sum(axis=1)), by_group('hospitalized'))
        assert np.array_equal(i64(r.pathway[:, 2]), by_group('in_icu')) and np.array_equal(i64(r.pathway[:, 1]), by_group('in_ward'))
        assert np.array_equal(i64(r.admissions.sum(axis=0)), by_group('hospitalized') + i64(r.pathway[:, [4, 5, 7, 8]].sum(axis=1)))
        assert int(r.admissions.sum()) == r.with_admission and int(r.icu_admissions.sum()) == r.with_icu
        assert int(r.pathway.sum()) == r.infected == int(by_group('all_infected').sum())
        assert np.array_equal(i64(r.pathway[:, :3].sum(axis=1)), by_group('infected'))
        assert int(r.deaths.sum() + r.recoveries.sum()) == r.with_outcome
        assert r.died_outside == int(by_group('non_hospital_deaths').sum())
        # the occupancy the history shows on day d + 1 is the admissions up to d less the outcomes of the admitted up to d
        det, adm, icu, out = ctx.course_log.days()
        occ = totals(hist, 'hospitalized')
        for d in (30, 90, 150, 199):
            assert int(((adm >= 0) & (adm < d) & ~((out >= 0) & (out < d))).sum()) == int(occ[d]), d
        # cohorts: every dated agent, and the log's own cohort sizes
        lr = ctx.transmission_log.report()
        assert np.array_equal(i64(r.cohort[..., 0].sum(axis=1)), i64(lr.cohort[..., 0].sum(axis=1)))
        assert np.array_equal(i64(r.cohort[..., 1].sum(axis=1)), i64(lr.cohort[..., 2].sum(axis=1)))
        assert int(r.cohort[..., 3].sum()) == int(by_group('dead').sum())


def test_context_routes_on_oracle_b_equal_run_host_driven(mini_200):
    ctx, hist, _ = mini_200
    v, ages = small_scenario()
    c = _oracle(v, ages, 3, course=True)
    assert c.transmission_log is not None and c.course_log is not None and not c.course_log.on_device
    h1 = c.run(120)                      # run() takes the host-driven route on a library without the entry points
    for _ in range(80):                  # ... and iterate() records too
        c.iterate()
    assert np.array_equal(h1, hist[:120])
    assert np.array_equal(c.course_log.words(), ctx.course_log.words())
    assert np.array_equal(c.transmission_log.words(), ctx.transmission_log.words())
    plain = _oracle(v, ages, 3)
    assert np.array_equal(plain.run(200), hist), 'a coursed run computes what a plain run computes'
    ll = c.transmission_log.line_list()
    r = c.course_log.report()
    assert {'detection_day', 'admission_day', 'icu_day', 'outcome_day'} <= set(ll.columns)
    assert int((ll['admission_day'] >= 0).sum()) == r.with_admission and int((ll['outcome_day'] >= 0).sum()) == r.with_outcome
    assert 'admission_day' not in plain.start_transmission_log().line_list().columns


def test_course_begun_at_day_60_marks_the_past_before(mini_200):
    ctx, hist, facts = mini_200
    v, ages = small_scenario()
    c = _oracle(v, ages, 3)
    c.run(60)
    c.start_course_log()                 # (begins the transmission log as well)
    assert c.transmission_log is not None and c.course_log.begin_day == 60
    h2 = c.run(140)
    assert np.array_equal(h2, hist[60:])
    want = cu.cut_records(ctx.course_log.words(), 60, facts.hot_at[60])
    got = c.course_log.words()
    bad = np.flatnonzero(got != want)
    assert not len(bad), [(int(i), hex(int(got[i])), hex(int(want[i]))) for i in bad[:5]]
    r = _report_equals_spec(c)
    assert int(r.pathway[:, 9].sum()) > 0


# ---------------------------------------------------------------------------------------------- 4. the header, the library

def _header():
    with open(os.path.join(ROOT, 'include', 'reina_course.h')) as fh:
        return fh.read()


def test_header_constants_and_offsets_equal_the_module():
    h = _header()
    defs = dict(re.findall(r'#define (REINA_COURSE_\w+) (.+?)(?:\s+/\*.*)?$', h, re.M))
    env = {'REINA_COURSE_S_NR': int(re.search(r'REINA_COURSE_S_NR = (\d+)', h).group(1))}
    for name, expr in defs.items():
        env[name] = eval(re.sub(r'\b(0x[0-9A-Fa-f]+|\d+)u\b', r'\1', expr), {}, env)
    assert env['REINA_COURSE_VERSION'] == crs.COURSE_VERSION
    for c in ('MAX_GROUPS', 'KINDS', 'DELAY_BINS', 'DETECTION_SHIFT', 'CLASSES', 'DAY_TABLES', 'COHORT_FIELDS', 'F_DETECTION',
              'F_ADMISSION', 'F_ICU', 'F_OUTCOME', 'DELAY', 'DELAY_N', 'DELAY_SUM', 'PATHWAY', 'SCALARS', 'FIXED_WORDS', 'DAY_WORDS'):
        assert env['REINA_COURSE_' + c] == getattr(crs, c), c
    assert crs.DAY_WORDS == 144 and crs.FIXED_WORDS == 8624
    macros = dict(re.findall(r'#define (REINA_COURSE_\w+)\(n_days\) (.+?)(?:\s+/\*.*)?$', h, re.M))
    order = ('DETECTIONS', 'ADMISSIONS', 'ICU_ADMISSIONS', 'DEATHS', 'RECOVERIES', 'COHORT', 'REPORT_WORDS')
    for n_days in (1, 365, eng.MAX_DAYS):
        fn = {}
        for name in order:
            e = macros['REINA_COURSE_' + name].replace('(size_t)', '')
            e = re.sub(r'(REINA_COURSE_\w+)\(n_days\)', lambda m: str(fn[m.group(1)]), e)
            fn['REINA_COURSE_' + name] = eval(e, dict(n_days=n_days), env)
        for k, name in enumerate(order[:-1]):
            assert fn['REINA_COURSE_' + name] == crs.day_table_offset(k, n_days), name
        assert fn['REINA_COURSE_REPORT_WORDS'] == crs.report_words(n_days)
    assert [n.upper() for n in crs.DAY_TABLE_NAMES] == list(order[:5])
    enum = re.search(r'enum \{(.*?)\};', h, re.S).group(1)
    names = [re.sub(r'\s*=.*', '', x).strip() for x in re.sub(r'/\*.*?\*/', '', enum, flags=re.S).split(',')]
    names = [x for x in names if x]
    assert names[:-1] == ['REINA_COURSE_S_' + s.upper() for s in crs.SCALAR_NAMES] and names[-1] == 'REINA_COURSE_S_NR'


def test_library_exports_every_function_the_header_declares():
    from reina_model_amd import build
    text = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    declared = sorted(set(re.findall(r'\b(reina_[a-z_]+)\s*\(', text)))
    assert declared == sorted('reina_' + f for f in crs.COURSE_FUNCTIONS)
    build.build()
    lib = eng.load_hip_library()
    for fn in declared:
        assert hasattr(lib, fn), fn
    f = crs.bind_course_abi(lib, 'reina_')
    assert f is not None and f['course_version']() == crs.COURSE_VERSION == 1
    assert eng.bind_abi(lib, 'reina_')['abi_version']() == 7
    assert crs.bind_course_abi(par_backend.lib(), 'par_') is None
    assert os.path.join(ROOT, 'include', 'reina_course.h') in build.DEPS


# ---------------------------------------------------------------------------------------------- 5. refusals (host side)

def test_refusals_on_the_host():
    from reina_model_amd import filtering, policy as pol
    v, ages = small_scenario()
    sharded = _oracle(v, ages, 1)
    sharded.n_shards = 2
    with pytest.raises(ValueError, match='sharded'):
        sharded.start_course_log()
    assert sharded.course_log is None and sharded.transmission_log is None
    c = _oracle(v, ages, 1, course=True)
    with pytest.raises(ValueError, match='already'):
        c.start_course_log()
    with pytest.raises(ValueError, match='transmission log'):
        c.snapshot()
    with pytest.raises(ValueError, match='transmission log'):
        filtering.FilterResult(c, [c], None, 0, c.start_date, 0)
    with pytest.raises(ValueError, match='transmission log'):
        c.restore(_oracle(v, ages, 1).snapshot())
    p = pol.Policy(pol.Signal('dead'), levels=[[], [['limit-mobility', 30]]], up=[2 ** 31 - 1], down=[0])
    with pytest.raises(ValueError, match='policy'):
        _oracle(v, ages, 1, ipc=None, policy=p, course=True)
    with pytest.raises(ValueError):
        c.course_log.report(n_days=eng.MAX_DAYS + 1)
    with pytest.raises(ValueError):
        c.course_log.report(n_days=0)

    class NoCourse:                       # an engine whose library has the log's entry points and not the course's
        course_f = None
    from reina_model_amd import reports
    with pytest.raises(eng.EngineError, match='reina_course.h'):
        reports.entry_points(NoCourse(), 'course_f', 'course-log', 'reina_course.h')
