"""The detection report on the CPU: the numpy specification (reina_model_amd/detection.py) against a plain per-agent and
per-link walker on synthetic states, conservation against the course, log and tree reports on oracle B, the model's own rules
of testing, tracing and quarantine, a course begun mid-run, the accessors on a hand-made state, the header against the module,
and the refusals.  Every comparison of words is of integers and exact."""
import os
import re

import numpy as np
import pytest

import course_util
import detection_util as du
import par_backend
import tx_util
from filter_util import small_scenario
from reina_model_amd import course as crs
from reina_model_amd import detection as det
from reina_model_amd import engine as eng
from reina_model_amd import simulation, txlog as txl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAYS = 200
NO, BF = txl.NONE, txl.BEFORE
i64 = lambda a: np.asarray(a).astype(np.int64)


# ---------------------------------------------------------------------------------------------- 1. report_numpy == walker

def _spec_and_walk(hot, inf, cnt, log, rec, n_days=du.N_DAYS, kind='default'):
    n = len(hot)
    age_start, g = tx_util.age_start_of(n), tx_util.groups(kind)
    r = det.report_numpy(hot, inf, cnt, log, rec, age_start, g, n_days)
    du.assert_words(r.words, du.walk_report(hot, inf, cnt, log, rec, age_start, [int(x) for x in g], n_days))
    return r


@pytest.mark.parametrize('n', (1, 511, 512, 513, 3 * 512 + 7))
def test_spec_equals_walker_on_random_states(n):
    hot, inf, cnt, log, rec = du.forest_state(n)
    r = _spec_and_walk(hot, inf, cnt, log, rec, kind='fine' if n % 2 else 'default')
    assert r.infected == int(((hot & 7) != 0).sum()) == r.roots + r.linked + r.bad_links
    if n > 500:
        assert r.bad_links > 0 and r.breach > 0 and (r.pair_class > 0).all(), 'bad links, breaches and every pair of classes occur'
    _spec_and_walk(hot, inf, cnt, log, rec, n_days=1)


def test_spec_equals_walker_on_every_combination():
    hot, inf, cnt, log, rec = du.combos_state()
    r = _spec_and_walk(hot, inf, cnt, log, rec)
    assert all(getattr(r, name) > 0 for name in det.SCALAR_NAMES), 'every scalar is hit'
    assert r.bad_links == 4, 'a self link, an infector out of range, a negative word, a susceptible infector'
    assert (r.ascertain.sum(axis=(0, 1)) > 0).all() and (r.phase.sum(axis=0) > 0).all(), 'every dc and every ph'
    assert (r.link_class.sum(axis=0) > 0).all(), 'every link class'
    assert (r.pair_class.sum(axis=1) > 0).all() and (r.pair_class.sum(axis=0) > 0).all()
    # RH_DETECTED set and clear against every det code: the record first
    d = crs.fields(rec)[0]
    infected, bit = (hot & 7) != 0, (hot & du.DETECTED) != 0
    for code, with_bit, without in ((NO, r.undated, r.never), (BF, None, None)):
        assert (infected & (d == code) & bit).any() and (infected & (d == code) & ~bit).any()
        if with_bit is not None:
            assert with_bit == int((infected & (d == code) & bit).sum()) and without == int((infected & (d == code) & ~bit).sum())
    assert (infected & (d < BF) & ~bit).any() and r.dated == int((infected & (d < BF)).sum()) and r.before == int((infected & (d == BF)).sum())
    # both ends of every clipped histogram, one bin inside and one beyond
    al, ld, pr = r.days_at_large().counts, r.lead_time().counts, r.pair_detection().counts
    assert al[0] >= 2 and al[63] >= 3 and ld[0] >= 1 and ld[63] >= 2, 'at_large: -1 on 0, 64 and 100 on 63; lead: 64 on 63'
    assert pr[0] >= 2 and pr[1] >= 1 and pr[126] >= 1 and pr[127] >= 2, 'pair: -65 on -64, +64 on +63'
    assert r.days_at_large().n == int(al.sum()) and int(r.at_large_sum.sum()) != int((al * np.arange(64)).sum()), 'the sum is taken before clipping'
    assert int(r.offspring[:, :, 63].sum()) > int(r.offspring[:, :, 62].sum()) > 0, 'n of 64 and 200 on top of 63'
    assert int(r.ascertain.sum()) == r.infected and int(r.link_class.sum()) == r.linked == int(r.pair_class.sum())
    assert int(r.link_class[:, 3].sum()) == r.breach
    one = _spec_and_walk(hot, inf, cnt, log, rec, n_days=1)
    assert one.out_of_range > r.out_of_range and np.array_equal(one.words[:det.SCALARS], r.words[:det.SCALARS]), 'the fixed tables take every agent'
    full = _spec_and_walk(hot, inf, cnt, log, rec, n_days=eng.MAX_DAYS, kind='fine')
    assert full.out_of_range == 0 and int(full.detections.sum()) == full.dated


def test_nothing_is_read_of_a_susceptible_agent():
    n = 700
    hot = np.full(n, du.DETECTED, dtype=np.uint32)              # flags, links, days and records of susceptible agents
    log = np.full(n, 5 << 16 | 3, dtype=np.uint32)
    r = _spec_and_walk(hot, np.zeros(n, dtype=np.int32), np.full(n, 7, dtype=np.int32), log, crs.pack([4] * n, [5] * n, [6] * n, [7] * n), n_days=10)
    assert not r.words.any()


# ---------------------------------------------------------------------------------------------- 2. simulated runs on oracle B

def _oracle(v, ages, seed, **kw):
    return simulation.make_context(v, age_counts=ages, seed=seed, ipc=None, engine_factory=par_backend.par_engine_factory, **kw)


@pytest.fixture(scope='module')
def tracing_200():
    v, ages = course_util.tracing_scenario()
    ctx = _oracle(v, ages, 3, course=True)
    assert not ctx.course_log.on_device and ctx.engine.detect_f is None
    ctx.run(DAYS)
    return ctx


def test_conservation_against_the_course_log_and_tree_reports(tracing_200):
    ctx = tracing_200
    r = ctx.course_log.detection_report()
    assert r == du.spec_report(ctx) and r.n_days == DAYS
    cr, lr, tr = ctx.course_log.report(), ctx.transmission_log.report(), ctx.transmission_report()
    hot = du.host_arrays(ctx)[0]
    assert int(r.ascertain.sum()) == r.infected == cr.infected
    assert int(r.ascertain[:, :, 1:].sum()) == int((((hot & 7) != 0) & ((hot & du.DETECTED) != 0)).sum())
    assert np.array_equal(i64(r.detections.sum(axis=1)), i64(cr.detections.sum(axis=1))), 'on every day'
    assert np.array_equal(i64(r.cohort[:, :, 0].sum(axis=1)), i64(lr.incidence.sum(axis=(1, 2))))
    assert r.linked == lr.links == tr.n_linked and r.bad_links == lr.bad_links == tr.bad_links == 0
    assert r.roots == lr.infected - lr.links - lr.bad_links == tr.n_roots
    assert int(r.link_class.sum()) == r.linked == int(r.pair_class.sum())
    assert int(r.offspring_sum.sum()) == int(tr.offspring_sum.sum()) == tr.sum_n_infected
    assert r.out_of_range == 0
    assert r.never + r.dated + r.before + r.undated == r.infected and r.before == 0 and r.undated == cr.detected_undated
    # n_days below the days run: the days beyond are counted, not dropped
    short = ctx.course_log.detection_report(n_days=50)
    assert short == du.spec_report(ctx, n_days=50) and short.out_of_range > 0
    assert np.array_equal(short.words[:det.SCALARS], r.words[:det.SCALARS]) and np.array_equal(short.cohort, r.cohort[:50])
    fine = ctx.course_log.detection_report(age_groups=np.minimum(np.arange(101) // 7, 15))
    assert fine == du.spec_report(ctx, groups=np.minimum(np.arange(101) // 7, 15)) and fine.n_groups == 15 and fine.linked == r.linked


# ---------------------------------------------------------------------------------------------- 3. the model's own rules

def test_the_quarantine_holds_and_tracing_shows(tracing_200):
    """A detected agent exposes nobody, tests run at the day's opening and a hospitalised agent has no contacts: no link is made
    after its infector's detection day.  Tracing detects before onset, detects asymptomatic agents, and finds an infectee the
    day after its infector."""
    r = tracing_200.course_log.detection_report()
    assert r.breach == 0 and r.linked > 1000
    assert int(r.phase[:, 0].sum()) > 0, 'detections before onset'
    assert int(r.ascertain[:, 0, det.DATED].sum()) > 0, 'detected asymptomatic agents'
    assert r.adjacent_share(1) > 0
    v, ages = small_scenario()
    plain = _oracle(v, ages, 3, course=True)
    plain.run(DAYS)
    p = plain.course_log.detection_report()
    assert p == du.spec_report(plain) and p.breach == 0 and p.linked > 1000 and p.dated > 0


def test_without_tracing_only_the_symptomatic_are_found_and_not_before_the_day_after_onset():
    """test-all-with-symptoms and never test-with-contact-tracing: only an agent with symptoms is queued for a test, the day it
    falls ill at the earliest, and the test runs at the next day's opening -- so nobody is detected before onset, no
    asymptomatic agent is ever detected, and a detection outside hospital comes a day after onset at the earliest."""
    v, ages = small_scenario()
    v['interventions'] = [iv for iv in v['interventions'] if not iv[0].startswith('test-')] + [['test-all-with-symptoms', '2020-02-18']]
    ctx = _oracle(v, ages, 3, course=True)
    ctx.run(DAYS)
    r = ctx.course_log.detection_report()
    assert r == du.spec_report(ctx) and r.dated > 1000 and r.breach == 0
    assert int(r.phase[:, 0].sum()) == 0
    assert int(r.ascertain[:, 0, det.DATED].sum()) == 0 and int(r.ascertain[:, 0].sum()) > 0
    d, adm, _, _ = crs.fields(ctx.course_log.words())
    o = i64(ctx.transmission_log.words() >> 16)
    outside = (d < BF) & ((adm == NO) | ((adm < BF) & (d < adm)))
    assert outside.sum() > 100 and (o[outside] < BF).all() and int((d - o)[outside].min()) >= 1
    assert int(r.phase[:, 2].sum()) == int(outside.sum())


# ---------------------------------------------------------------------------------------------- 4. a course begun mid-run

def test_course_begun_at_day_60_counts_earlier_detections_before_and_their_links_undetermined(tracing_200):
    full = tracing_200
    v, ages = course_util.tracing_scenario()
    c = _oracle(v, ages, 3, txlog=True)
    c.run(60)
    hot60 = du.host_arrays(c)[0]
    c.start_course_log()
    c.run(DAYS - 60)
    assert np.array_equal(du.host_arrays(c)[0], du.host_arrays(full)[0])
    r, f = c.course_log.detection_report(), full.course_log.detection_report()
    assert r == du.spec_report(c)
    detected60 = ((hot60 & 7) != 0) & ((hot60 & du.DETECTED) != 0)
    early = detected60 | ((hot60 & 7) >= 5)          # (the begin pass closes the record of an agent removed by then: BEFORE throughout)
    assert r.before == int(early.sum()) > int(detected60.sum()) > 0, 'agents detected, or removed, before the course began'
    hot, k = du.host_rows(c)
    s = k.s[k.linked]
    assert int(r.link_class[:, 4].sum()) >= int(early[s].sum()) > 0, 'their links are undetermined'
    assert int(r.pair_class[det.BEFORE_COURSE].sum()) == int(early[s].sum())
    assert r.breach == 0
    assert r.infected == f.infected and r.linked == f.linked and np.array_equal(r.cohort[:, :, 0], f.cohort[:, :, 0])
    assert int(r.detections[:60].sum()) == 0 and np.array_equal(r.detections[61:].sum(axis=1), f.detections[61:].sum(axis=1))


# ---------------------------------------------------------------------------------------------- 5. accessors

def _hand_made():
    """Eleven infected agents and a susceptible one; the agents 0-5 are of age 10 (group 1), 6-11 of age 50 (group 5).
       i  st sev DET   t   o  det adm  infector n   dc      ph  link (class, lead)        pair
       0   5  1   x   10  14  16   -     -      3   dated   2   root
       1   5  0   x   12   -  17   -     0      0   dated   0   1, lead 4                 +1
       2   6  4   x   16  18  20  20     0      0   dated   1   2, lead 0                 +4
       3   2  1   .   15  19   -   -     0      0   never       1, lead 1
       4   5  1   .    5   9   -   -     -      2   never       root
       5   5  2   x    8  12  13  15     4      2   dated   2   0 (infector never found)
       6   5  0   .    9   -   -   -     4      0   never       0
       7   5  1   x   13  16  14   -     5      0   dated   0   2, lead 0                 +1
       8   1  0   .   12   -   -   -     5      0   never       1, lead 1
       9   5  1   x    B   B   B   -     -      1   before      root
      10   5  1   x   30  33   -   -     9      0   undated     4 (infector's day unknown)
    n_days = 21: agent 10's t = 30 is out of range."""
    rows = [(5, 1, 1, 10, 14, 16, NO, -1, 3), (5, 0, 1, 12, NO, 17, NO, 0, 0), (6, 4, 1, 16, 18, 20, 20, 0, 0), (2, 1, 0, 15, 19, NO, NO, 0, 0),
            (5, 1, 0, 5, 9, NO, NO, -1, 2), (5, 2, 1, 8, 12, 13, 15, 4, 2), (5, 0, 0, 9, NO, NO, NO, 4, 0), (5, 1, 1, 13, 16, 14, NO, 5, 0),
            (1, 0, 0, 12, NO, NO, NO, 5, 0), (5, 1, 1, BF, BF, BF, NO, -1, 1), (5, 1, 1, 30, 33, NO, NO, 9, 0), (0, 0, 0, NO, NO, NO, NO, -1, 0)]
    a = np.array(rows, dtype=np.int64)
    hot = (a[:, 0] | a[:, 1] << 3 | a[:, 2] * du.DETECTED).astype(np.uint32)
    log = (a[:, 4] << 16 | a[:, 3]).astype(np.uint32)
    rec = crs.pack(a[:, 5], a[:, 6], [NO] * 12, [NO] * 12)
    age_start = np.full(eng.MAX_AGES + 1, 12, dtype=np.int64)
    age_start[:11], age_start[11:51] = 0, 6
    r = det.report_numpy(hot, a[:, 7].astype(np.int32), a[:, 8].astype(np.int32), log, rec, age_start, tx_util.groups(), 21)
    labels = ['0-9', '10-19', '20-29', '30-39', '40-49', '50-59', '60-69', '70-79', '80+']
    return det.DetectionReport(r.words, 21, 9, labels, '2021-03-01')


def test_report_accessors_on_a_hand_made_state():
    r = _hand_made()
    assert (r.infected, r.roots, r.linked, r.bad_links, r.never, r.dated, r.before, r.undated, r.breach, r.out_of_range) == (11, 3, 8, 0, 4, 5, 1, 1, 0, 1)
    a = r.ascertainment_frame()
    assert a.shape == (72, 3) and a.index.names == ['age_group', 'severity']
    assert tuple(a.loc[('10-19', 'mild')]) == (1 / 3, 1, 3) and tuple(a.loc[('10-19', 'asymptomatic')]) == (1.0, 1, 1)
    assert tuple(a.loc[('50-59', 'asymptomatic')]) == (0.0, 0, 2) and tuple(a.loc[('50-59', 'mild')]) == (1.0, 3, 3)
    assert np.isnan(a.loc[('50-59', 'severe'), 'share']) and a.loc[('50-59', 'severe'), 'infected'] == 0, 'an empty cell has no share'
    c = r.ascertainment_by_cohort()
    assert c.shape == (21, 3) and str(c.index[0])[:10] == '2021-03-01'
    assert tuple(c.iloc[12]) == (0.5, 2, 0.5) and tuple(c.iloc[5]) == (0.0, 1, 1.0) and tuple(c.iloc[8]) == (1.0, 1, 1.0)
    assert np.isnan(c.iloc[0, 0]) and c.iloc[0, 1] == 0 and np.isnan(c.iloc[0, 2]), 'an empty day'
    assert tuple(r.ascertainment_by_cohort(group=5).iloc[12]) == (0.0, 1, 0.0) and int(c['cohort'].sum()) == 9
    d = r.detections_frame()
    assert d.shape == (21, 4) and list(d.columns) == list(det.PHASE_NAMES)
    assert [list(d.iloc[k]) for k in (13, 14, 16, 17, 20)] == [[0, 0, 1, 0], [1, 0, 0, 0], [0, 0, 1, 0], [1, 0, 0, 0], [0, 1, 0, 0]] and int(d.values.sum()) == 5
    p = r.phase_frame()
    assert list(p.loc['10-19']) == [1, 1, 2, 0] and list(p.loc['50-59']) == [1, 0, 0, 0] and p.shape == (9, 4)
    al = r.days_at_large()
    assert (al.n, al.sum, al.mean(), al.total()) == (5, 21, 4.2, 5) and al.counts[5] == 2 and al.quantile(0.5) == 5
    assert r.days_at_large(group=1).mean() == 5.0 and r.days_at_large(group=5).mean() == 1.0 and r.days_at_large(group=0).mean() is None
    o = r.offspring_by_detection()
    assert list(o.index) == list(det.CLASS_NAMES)
    assert list(o[('all', 'mean')]) == [0.5, 1.0, 1.0, 0.0] and list(o[('all', 'agents')]) == [4, 5, 1, 1] and list(o[('all', 'offspring')]) == [2, 5, 1, 0]
    assert list(o[('closed', 'mean')]) == [1.0, 1.0, 1.0, 0.0] and list(o[('closed', 'agents')]) == [2, 5, 1, 1]
    assert r.transmission_share('never') == (0.25, 2, 8) and r.transmission_share('never', closed_only=True) == (0.25, 2, 8)
    assert r.transmission_share(det.DATED) == (0.625, 5, 8) and r.transmission_share('undated') == (0.0, 0, 8)
    lf = r.link_frame()
    assert list(lf.columns) == list(det.LINK_CLASS_NAMES) and list(lf.loc['10-19']) == [2, 3, 2, 0, 0] and list(lf.loc['50-59']) == [0, 0, 0, 0, 1]
    lt = r.lead_time()
    assert (lt.total(), lt.mean(), lt.counts[0], lt.counts[1], lt.counts[4]) == (5, 1.2, 2, 2, 1) and r.lead_time(group=5).mean() is None
    assert r.averted_if_earlier(1) == (0.4, 2, 5) and r.averted_if_earlier(4) == (0.6, 3, 5) and r.averted_if_earlier(0) == (0.0, 0, 5)
    assert r.averted_if_earlier(1000) == (0.6, 3, 5)
    with pytest.raises(ValueError):
        r.averted_if_earlier(-1)
    pd_ = r.pair_detection()
    assert pd_.total() == 3 and pd_.mean() == 2.0 and pd_.series().index[0] == -64 and len(pd_.counts) == 128
    assert r.adjacent_share(1) == 2 / 3 and r.adjacent_share(4) == 1 / 3 and r.adjacent_share(0) == 0.0 and r.adjacent_share(-1) == 2 / 3
    pf = r.pair_frame()
    assert [list(pf.loc[k]) for k in det.CLASS_NAMES] == [[1, 1, 0, 0], [2, 3, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0]]
    lk = r.links_frame()
    assert tuple(lk.iloc[12]) == (2, 0, 2, 0.0) and tuple(lk.iloc[8]) == (1, 1, 0, 1.0) and tuple(lk.iloc[16]) == (1, 0, 1, 0.0)
    assert np.isnan(lk.iloc[0, 3]) and lk.iloc[0, 0] == 0 and int(lk['links'].sum()) == 7, 'the link on day 30 is out of range'
    assert 'breach=0' in repr(r) and 'never=4' in repr(r)
    assert r == det.DetectionReport(r.words.copy(), 21, 9) and r != det.DetectionReport(np.zeros_like(r.words), 21, 9)
    with pytest.raises(ValueError, match='words'):
        det.DetectionReport(r.words, 22)
    # an empty report: every empty class gives None
    e = det.DetectionReport(np.zeros(det.report_words(3), dtype=np.uint64), 3)
    assert e.days_at_large().mean() is None and e.lead_time().mean() is None and e.pair_detection().mean() is None
    assert e.transmission_share('never') == (None, 0, 0) and e.averted_if_earlier(3) == (None, 0, 0) and e.adjacent_share() is None
    assert np.isnan(e.offspring_by_detection()[('all', 'mean')]).all() and list(e.detections_frame().index) == [0, 1, 2]
    assert np.isnan(e.links_frame()['never_share']).all() and e.ascertainment_frame().shape == (128, 3)


# ---------------------------------------------------------------------------------------------- 6. the header, the library

def _header():
    with open(os.path.join(ROOT, 'include', 'reina_detection.h')) as fh:
        return fh.read()


def test_header_constants_and_offsets_equal_the_module():
    h = _header()
    defs = dict(re.findall(r'#define (REINA_DETECT_\w+) (.+?)(?:\s+/\*.*)?$', h, re.M))
    env = {'REINA_DETECT_S_NR': int(re.search(r'REINA_DETECT_S_NR = (\d+)', h).group(1))}
    for name, expr in defs.items():
        env[name] = eval(re.sub(r'\b(0x[0-9A-Fa-f]+|\d+)u\b', r'\1', expr), {}, env)
    assert env['REINA_DETECT_VERSION'] == det.DETECT_VERSION
    for c in ('MAX_GROUPS', 'SEVERITIES', 'CLASSES', 'PHASES', 'LINK_CLASSES', 'BINS', 'PAIR_BINS', 'PAIR_SHIFT', 'COHORT_FIELDS', 'LINK_DAY_FIELDS',
              'NEVER', 'DATED', 'UNDATED', 'ASCERTAIN', 'PHASE', 'AT_LARGE', 'AT_LARGE_N', 'AT_LARGE_SUM', 'OFFSPRING', 'OFFSPRING_SUM',
              'LINK_CLASS', 'LEAD', 'PAIR', 'PAIR_CLASS', 'SCALARS', 'FIXED_WORDS', 'DAY_WORDS'):
        assert env['REINA_DETECT_' + c] == getattr(det, c), c
    assert env['REINA_DETECT_BEFORE'] == det.BEFORE_COURSE == 2
    assert det.DAY_WORDS == 55 and det.FIXED_WORDS == 3416 and det.MAX_GROUPS == txl.MAX_GROUPS == crs.MAX_GROUPS
    macros = dict(re.findall(r'#define (REINA_DETECT_\w+)\(n_days\) (.+?)(?:\s+/\*.*)?$', h, re.M))
    order = ('COHORT', 'DETECTIONS', 'LINKS_BY_DAY', 'REPORT_WORDS')
    for n_days in (1, 365, eng.MAX_DAYS):
        fn = {}
        for name in order:
            e = macros['REINA_DETECT_' + name].replace('(size_t)', '')
            e = re.sub(r'(REINA_DETECT_\w+)\(n_days\)', lambda m: str(fn[m.group(1)]), e)
            fn['REINA_DETECT_' + name] = eval(e, dict(n_days=n_days), env)
        assert fn['REINA_DETECT_COHORT'] == det.cohort_offset(n_days) and fn['REINA_DETECT_DETECTIONS'] == det.detections_offset(n_days)
        assert fn['REINA_DETECT_LINKS_BY_DAY'] == det.links_by_day_offset(n_days) and fn['REINA_DETECT_REPORT_WORDS'] == det.report_words(n_days)
    enum = re.search(r'enum \{(.*?)\};', h, re.S).group(1)
    names = [re.sub(r'\s*=.*', '', x).strip() for x in re.sub(r'/\*.*?\*/', '', enum, flags=re.S).split(',')]
    names = [x for x in names if x]
    assert names[:-1] == ['REINA_DETECT_S_' + s.upper() for s in det.SCALAR_NAMES] and names[-1] == 'REINA_DETECT_S_NR'


def test_library_exports_every_function_the_header_declares():
    from reina_model_amd import build
    text = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    declared = sorted(set(re.findall(r'\b(reina_[a-z_]+)\s*\(', text)))
    assert declared == sorted('reina_' + f for f in det.DETECT_FUNCTIONS)
    build.build()
    lib = eng.load_hip_library()
    for fn in declared:
        assert hasattr(lib, fn), fn
    f = det.bind_detect_abi(lib, 'reina_')
    assert f is not None and f['detect_version']() == det.DETECT_VERSION == 1
    assert eng.bind_abi(lib, 'reina_')['abi_version']() == 7
    assert det.bind_detect_abi(par_backend.lib(), 'par_') is None
    assert os.path.join(ROOT, 'include', 'reina_detection.h') in build.DEPS
    with open(os.path.join(ROOT, 'include', 'reina_hip.h')) as fh:
        assert 'reina_detect' not in fh.read(), 'nothing is added to reina_hip.h'


# ---------------------------------------------------------------------------------------------- 7. refusals (host side)

def test_refusals_on_the_host(tracing_200):
    from reina_model_amd import ensemble, reports
    ctx = tracing_200
    for n_days in (0, eng.MAX_DAYS + 1):
        with pytest.raises(ValueError, match='n_days'):
            ctx.course_log.detection_report(n_days=n_days)
        with pytest.raises(ValueError, match='n_days'):
            det.report_numpy(np.zeros(4, dtype=np.uint32), np.zeros(4, dtype=np.int32), np.zeros(4, dtype=np.int32), np.zeros(4, dtype=np.uint32),
                             np.zeros(4, dtype=np.uint64), tx_util.age_start_of(4), tx_util.groups(), n_days)
    with pytest.raises(ValueError, match='age groups'):
        ctx.course_log.detection_report(age_groups=np.arange(101) // 5)                  # (groups up to 20)
    v, ages = small_scenario()
    logged = _oracle(v, ages, 1, txlog=True)                                             # a transmission log and no course
    assert logged.course_log is None
    with pytest.raises(ValueError, match='no course log'):
        ensemble.detection_reports([logged])
    with pytest.raises(ValueError, match='no course log'):
        ensemble.detection_reports([ctx, _oracle(v, ages, 1)])

    class NoDetect:                        # an engine whose library has the course's entry points and not the report's
        detect_f = None
    with pytest.raises(eng.EngineError, match='reina_detection.h'):
        reports.entry_points(NoDetect(), 'detect_f', 'detection report', 'reina_detection.h')

    class Course:                          # ... and its device course: the device route says so instead of falling back
        engine, members, engines, group, _h = NoDetect(), 1, (), None, None
    with pytest.raises(eng.EngineError, match='reina_detection.h'):
        det.device_report_words(Course(), np.zeros(eng.MAX_AGES, dtype=np.uint8), 1, 4)
    # contexts with courses of their own are reported one by one
    reps = ensemble.detection_reports([ctx, ctx], n_days=30)
    assert len(reps) == 2 and reps[0] == reps[1] == ctx.course_log.detection_report(n_days=30)
