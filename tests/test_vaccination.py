"""The vaccination report on the CPU: the numpy specification (reina_model_amd/vaccination.py) against a plain per-agent walker
on synthetic states, conservation against the engine's own counters and the transmission log's report on oracle B, a log begun
mid-run, the accessors on a hand-made block, the header against the module, the refusals, and the protection a programme
realises on oracle B.  Every comparison of words is of integers and exact."""
import os
import re

import numpy as np
import pytest

import par_backend
import tx_util
import vacc_util as vu
from filter_util import small_scenario, totals
from reina_model_amd import engine as eng
from reina_model_amd import simulation, txlog as txl
from reina_model_amd import vaccination as vac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAYS = 200
i64 = lambda a: np.asarray(a).astype(np.int64)


# ---------------------------------------------------------------------------------------------- 1. report_numpy == walker

def _spec_and_walk(hot, vd, log, n_days=vu.N_DAYS, kind='default'):
    n = len(hot)
    age_start, g = tx_util.age_start_of(n), tx_util.groups(kind)
    r = vac.report_numpy(hot, vd, log, age_start, g, n_days)
    vu.assert_words(r.words, vu.walk_report(hot, vd, log, age_start, [int(x) for x in g], n_days))
    return r


@pytest.mark.parametrize('n', (1, 511, 512, 513, 3 * 512 + 7))
def test_spec_equals_walker_on_random_states(n):
    hot, _, _, log, vd = vu.forest_state(n)
    r = _spec_and_walk(hot, vd, log, kind='fine' if n % 2 else 'default')
    assert r.vaccinated == int(((hot & vu.VACCINATED) != 0).sum()) and r.infected == int(((hot & 7) != 0).sum())


def test_spec_equals_walker_on_every_combination():
    hot, _, _, log, vd = vu.combos_state()
    r = _spec_and_walk(hot, vd, log)
    assert (r.outcome[:, :, 0].sum(axis=1) > 0).all(), 'every status occurs'
    assert all(getattr(r, name) > 0 for name in vac.SCALAR_NAMES), 'every scalar is hit'
    assert (r.severity.sum(axis=1)[:, :5] > 0).all() and not r.severity[:, :, 5:].any(), 'every status x severity 0..4'
    s = r.since_vaccination().counts
    assert s[0] > 0 and s[14] > 0 and s[15] > 0 and s[127] >= 2 * s[15], 'both ends of the histogram, and the clipped 128 on top of 127'
    assert int(r.outcome[vac.RECENT, :, 0].sum()) == int(r.since[0, :, :15].sum()), 'recent is 0..14 days'
    assert int(r.outcome[vac.PROTECTED, :, 0].sum()) == int(r.since[0, :, 15:].sum())
    assert int(r.vaccinations.sum()) + r.bad_vacc_day < r.vaccinated, 'valid days beyond n_days are out of range'
    assert int(r.population[:, 1].sum()) > 0 and int(r.population[:, 1:].sum()) == r.vaccinated == int(r.population[:, 0].sum())
    assert int(r.outcome[:, :, 0].sum()) == r.infected and int(r.outcome[vac.UNDETERMINED, :, 0].sum()) == r.undetermined
    one = _spec_and_walk(hot, vd, log, n_days=1)
    assert one.out_of_range > r.out_of_range and np.array_equal(one.words[:vac.SCALARS], r.words[:vac.SCALARS]), 'the fixed tables take every agent'
    full = _spec_and_walk(hot, vd, log, n_days=eng.MAX_DAYS, kind='fine')
    assert full.out_of_range == 0 and int(full.vaccinations.sum()) + full.bad_vacc_day == full.vaccinated


def test_nothing_is_read_of_an_agent_that_is_neither():
    n = 700
    hot = np.zeros(n, dtype=np.uint32)
    log = np.full(n, 5 << 16 | 3, dtype=np.uint32)            # log words and vaccination days of susceptible unvaccinated agents
    r = _spec_and_walk(hot, np.full(n, 7, dtype=np.int32), log, n_days=10)
    assert not r.words.any()


# ---------------------------------------------------------------------------------------------- 2. simulated runs on oracle B

def _oracle(v, ages, seed, **kw):
    return simulation.make_context(v, age_counts=ages, seed=seed, ipc=None, engine_factory=par_backend.par_engine_factory, **kw)


@pytest.fixture(scope='module')
def mini_200():
    v, ages = vu.vaccination_scenario()
    ctx = _oracle(v, ages, 3, txlog=True)
    assert not ctx.transmission_log.on_device and ctx.engine.vacc_f is None
    hist = ctx.run(DAYS)
    return ctx, hist


def test_conservation_against_the_engines_counters(mini_200):
    ctx, hist = mini_200
    r = ctx.transmission_log.vaccination_report()
    assert r == vu.spec_report(ctx) and r.n_days == DAYS
    final = np.asarray(ctx.engine.read_counters())
    table = np.asarray(ctx._tx_groups(None)[0])[:ctx.nr_ages]

    def by_group(row, name):
        ci = eng.C_NAMES.index(name)
        c = np.asarray(row)[ci * eng.MAX_AGES:ci * eng.MAX_AGES + ctx.nr_ages].astype(np.int64)
        return np.bincount(table, weights=c, minlength=vac.MAX_GROUPS).astype(np.int64)

    assert np.array_equal(i64(r.vaccinations.sum(axis=0)), by_group(final, 'vaccinated'))
    assert np.array_equal(i64(r.population[:, 0]), by_group(final, 'vaccinated'))
    cum = np.concatenate([np.zeros((1, vac.MAX_GROUPS), dtype=np.int64), np.cumsum(i64(r.vaccinations), axis=0)])   # cum[d]: vd < d
    for d in range(DAYS):
        assert np.array_equal(cum[d], by_group(hist[d], 'vaccinated')), d
    assert np.array_equal(i64(r.outcome[:, :, 0].sum(axis=0)), by_group(final, 'all_infected'))
    assert np.array_equal(i64(r.outcome[:, :, 2].sum(axis=0)), by_group(final, 'dead'))
    lr = ctx.transmission_log.report()
    assert np.array_equal(i64(r.infections.sum(axis=2)), i64(lr.incidence.sum(axis=1)))
    assert np.array_equal(i64(r.cohort[:, :, 0].sum(axis=1)), i64(lr.cohort[:, :, 0].sum(axis=1)))
    assert np.array_equal(i64(r.cohort[:, :, 3].sum(axis=1)), i64(lr.cohort[:, :, 2].sum(axis=1)))
    assert r.undetermined == r.bad_vacc_day == r.out_of_range == 0
    assert r.vaccinated == int(totals(final[None], 'vaccinated')[0]) and r.infected == lr.infected
    # not vacuous: both kinds of breakthrough, vaccinations after an infection, and the second programme's overlapping window
    recent, protected = int(r.outcome[vac.RECENT, :, 0].sum()), int(r.outcome[vac.PROTECTED, :, 0].sum())
    assert recent > 500 and protected > 1000 and r.after_infection > 500
    assert int(r.vaccinations[:50, 1:3].sum()) == 0 and int(r.vaccinations[50:, 1:3].sum()) > 1000, 'the ages 10..29 are reached from day 50 on'
    assert int(r.vaccinations[:10].sum()) == 0 and int(r.vaccinations[10].sum()) == 1000
    assert r.doses_frame().index[10].isoformat()[:10] == vu.day_date(10)
    # n_days below the days run: the days beyond are counted, not dropped
    short = ctx.transmission_log.vaccination_report(n_days=50)
    assert short == vu.spec_report(ctx, n_days=50) and short.out_of_range > 0
    assert np.array_equal(short.words[:vac.SCALARS], r.words[:vac.SCALARS])
    assert np.array_equal(short.vaccinations, r.vaccinations[:50]) and np.array_equal(short.infections, r.infections[:50])


def test_log_begun_at_day_60_dates_the_vaccinations_and_not_the_earlier_infections(mini_200):
    ctx, hist = mini_200
    v, ages = vu.vaccination_scenario()
    c = _oracle(v, ages, 3)
    c.run(60)
    c.start_transmission_log()
    assert np.array_equal(c.run(DAYS - 60), hist[60:])
    r, full = c.transmission_log.vaccination_report(), ctx.transmission_log.vaccination_report()
    assert r == vu.spec_report(c)
    hot, vd = vu.host_arrays(ctx)
    assert np.array_equal(hot, vu.host_arrays(c)[0])
    t = ctx.transmission_log.infection_day()
    inf, vaccinated = (hot & 7) != 0, (hot & vu.VACCINATED) != 0
    assert (t[inf] >= 0).all()
    assert np.array_equal(r.vaccinations, full.vaccinations) and int(r.vaccinations[:60].sum()) > 0, 'vaccination days before the log began are dated'
    early = inf & (t < 60)
    assert r.undetermined == int((early & vaccinated).sum()) > 0, 'vaccinated agents infected before the log began'
    late_after = inf & vaccinated & (t >= 60) & (vd > t)
    assert r.after_infection == int(late_after.sum())
    assert int(r.outcome[vac.UNVACCINATED, :, 0].sum()) == int((inf & ~vaccinated).sum()) + r.after_infection, 'the unvaccinated stay status 0'
    assert int(r.infections[:60].sum()) == 0 and np.array_equal(r.infections[60:, :, 1:], full.infections[60:, :, 1:])
    assert int((early & ~vaccinated).sum()) > 0


# ---------------------------------------------------------------------------------------------- 3. accessors

def _hand_made():
    """a block of 6 days and 3 groups with known cells"""
    n_days = 6
    w = np.zeros(vac.report_words(n_days), dtype=np.uint64)
    sev = w[vac.SEVERITY:vac.OUTCOME].reshape(4, 16, 8)
    out = w[vac.OUTCOME:vac.SINCE].reshape(4, 16, 4)
    since = w[vac.SINCE:vac.POPULATION].reshape(2, 16, 128)
    pop = w[vac.POPULATION:vac.SCALARS].reshape(16, 3)
    a, b, c = vac.vaccinations_offset(n_days), vac.infections_offset(n_days), vac.cohort_offset(n_days)
    doses = w[a:b].reshape(n_days, 16)
    infs = w[b:c].reshape(n_days, 16, 3)
    coh = w[c:].reshape(n_days, 3, 4)
    sev[0, 1] = [50, 30, 12, 6, 2, 0, 0, 0]         # group 1, unvaccinated: 100 agents, 20 severe or worse
    sev[2, 1] = [120, 76, 3, 1, 0, 0, 0, 0]         # group 1, protected: 200 agents, 4 severe or worse
    sev[0, 2] = [10, 0, 0, 0, 0, 0, 0, 0]           # group 2, unvaccinated: nobody severe
    sev[2, 2] = [10, 0, 1, 0, 0, 0, 0, 0]
    out[0, 1] = [100, 80, 8, 40]
    out[2, 1] = [200, 100, 1, 30]
    out[2, 2] = [11, 0, 0, 0]                       # nobody closed
    since[0, 1, 3], since[0, 1, 20], since[1, 1, 3] = 5, 15, 2
    pop[1], pop[2] = [300, 100, 200], [20, 9, 11]
    doses[1, 1], doses[3, 1], doses[2, 2] = 100, 200, 20
    infs[4, 1] = [6, 1, 3]
    infs[5, 2, 0] = 2
    coh[4] = [[6, 2, 1, 5], [1, 0, 0, 1], [3, 1, 0, 2]]
    w[vac.SCALARS:vac.SCALARS + 7] = [320, 321, 211, 4, 5, 0, 7]
    return vac.VaccinationReport(w, n_days, 3, ['young', 'middle', 'old'], '2021-03-01', group_sizes=[0, 400, 40] + [0] * 13)


def test_report_accessors_on_a_hand_made_block():
    r = _hand_made()
    assert (r.vaccinated, r.infected, r.vaccinated_infected, r.after_infection, r.undetermined, r.bad_vacc_day, r.out_of_range) == (320, 321, 211, 4, 5, 0, 7)
    d = r.doses_frame()
    assert d.shape == (6, 3) and list(d.columns) == ['young', 'middle', 'old'] and d.columns.name == 'age_group'
    assert str(d.index[0])[:10] == '2021-03-01' and int(d.loc[d.index[3], 'middle']) == 200
    c = r.coverage_frame()
    assert c.shape == (6, 3) and list(c['middle']) == [0.0, 0.25, 0.25, 0.75, 0.75, 0.75] and c['old'].iloc[-1] == 0.5
    assert np.isnan(c['young']).all(), 'an empty group has no coverage'
    assert int(r.infections_frame().iloc[4].sum()) == 10 and int(r.infections_frame('protected').iloc[4, 1]) == 3
    assert int(r.infections_frame(0).values.sum()) == 8
    with pytest.raises(ValueError):
        r.infections_frame('undetermined')
    b = r.breakthrough_share()
    assert b.iloc[4] == 0.4 and b.iloc[5] == 0.0 and np.isnan(b.iloc[0]) and b.shape == (6,)
    s = r.severity_frame()
    assert s.shape == (4, 8) and list(s.index) == list(vac.STATUS_NAMES) and list(s.columns)[:5] == ['asymptomatic', 'mild', 'severe', 'critical', 'fatal']
    assert int(s.loc['unvaccinated', 'severe']) == 12 and int(r.severity_frame(group=2).loc['protected', 'severe']) == 1
    assert r.severe_share('unvaccinated', 1) == (0.2, 100) and r.severe_share(vac.PROTECTED, 1) == (0.02, 200)
    assert r.severe_share('recent') == (None, 0)
    p = r.protection_against_severe(1)
    assert p.protection == pytest.approx(0.9) and (p.protected_count, p.unvaccinated_count) == (200, 100) and (p.protected_share, p.unvaccinated_share) == (0.02, 0.2)
    assert r.protection_against_severe(2).protection is None and r.protection_against_severe(2).unvaccinated_share == 0.0, 'no unvaccinated agent is severe'
    assert r.protection_against_severe(0) == (None, None, 0, None, 0)
    allg = r.protection_against_severe()
    assert allg.protected_count == 211 and allg.unvaccinated_count == 110 and allg.protection == pytest.approx(1 - (5 / 211) / (20 / 110))
    q = r.protection_against_death(1)
    assert q.protection == pytest.approx(0.9) and (q.protected_count, q.unvaccinated_count) == (100, 80)
    assert (q.protected_share, q.unvaccinated_share, q.protected_closed_share, q.unvaccinated_closed_share) == (0.01, 0.1, 0.5, 0.8)
    z = r.protection_against_death(2)
    assert z.protection is None and z.protected_share is None and z.protected_closed_share == 0.0 and z.unvaccinated_closed_share is None
    iv = r.since_vaccination(group=1)
    assert iv.total() == 20 and iv.mean() == (5 * 3 + 15 * 20) / 20 and iv.series().index[0] == 0 and len(iv.counts) == 128
    assert r.since_vaccination(severe=True).total() == 2 and r.since_vaccination(group=0).mean() is None
    k = r.protection_by_cohort()
    assert k.shape == (6, 12) and list(k.columns[:4]) == [('unvaccinated', f) for f in ('agents', 'severe', 'dead', 'closed')]
    assert list(k.iloc[4]) == [6, 2, 1, 5, 1, 0, 0, 1, 3, 1, 0, 2]
    assert list(r.population_frame().loc['middle']) == [300, 100, 200] and list(r.outcome_frame(1).loc['protected']) == [200, 100, 1, 30]
    assert 'vaccinated=320' in repr(r)
    assert r == vac.VaccinationReport(r.words.copy(), 6, 3) and r != vac.VaccinationReport(np.zeros_like(r.words), 6, 3)
    with pytest.raises(ValueError, match='words'):
        vac.VaccinationReport(r.words, 7)
    with pytest.raises(ValueError, match='group sizes'):
        vac.VaccinationReport(r.words, 6).coverage_frame()
    days = vac.VaccinationReport(r.words, 6)
    assert list(days.doses_frame().index) == list(range(6)) and days.doses_frame().shape == (6, 16)


def test_coverage_against_the_group_sizes_of_a_population(mini_200):
    ctx, _ = mini_200
    r = ctx.transmission_log.vaccination_report()
    table = np.asarray(ctx._tx_groups(None)[0])[:ctx.nr_ages]
    sizes = np.bincount(table, weights=np.diff(np.asarray(ctx.age_start)[:ctx.nr_ages + 1]), minlength=16).astype(np.int64)
    assert np.array_equal(r.group_sizes, sizes) and int(sizes.sum()) == ctx.engine.config.n_agents
    c = r.coverage_frame()
    assert c.shape == (DAYS, r.n_groups) and list(c.columns) == list(ctx.age_group_labels)
    assert np.allclose(c.iloc[-1].values, i64(r.population[:r.n_groups, 0]) / sizes[:r.n_groups])
    assert c.iloc[-1, 0] == 0.0 and 0.9 < c.iloc[-1, 5] <= 1.0 and (np.diff(c.values, axis=0) >= 0).all()   # (the dead are not vaccinated)
    fine = ctx.transmission_log.vaccination_report(age_groups=np.minimum(np.arange(101) // 7, 15))
    assert fine == vu.spec_report(ctx, groups=np.minimum(np.arange(101) // 7, 15)) and fine.n_groups == 15
    assert int(fine.vaccinations.sum()) == int(r.vaccinations.sum())


# ---------------------------------------------------------------------------------------------- 4. the header, the library

def _header():
    with open(os.path.join(ROOT, 'include', 'reina_vaccination.h')) as fh:
        return fh.read()


def test_header_constants_and_offsets_equal_the_module():
    h = _header()
    defs = dict(re.findall(r'#define (REINA_VACC_\w+) (.+?)(?:\s+/\*.*)?$', h, re.M))
    env = {'REINA_VACC_S_NR': int(re.search(r'REINA_VACC_S_NR = (\d+)', h).group(1))}
    for name, expr in defs.items():
        env[name] = eval(re.sub(r'\b(0x[0-9A-Fa-f]+|\d+)u\b', r'\1', expr), {}, env)
    assert env['REINA_VACC_VERSION'] == vac.VACC_VERSION
    for c in ('MAX_GROUPS', 'STATUSES', 'DATED_STATUSES', 'PROTECTION_DAYS', 'SEVERITIES', 'OUTCOME_FIELDS', 'SINCE_KINDS', 'SINCE_BINS',
              'POPULATION_FIELDS', 'COHORT_FIELDS', 'UNVACCINATED', 'RECENT', 'PROTECTED', 'UNDETERMINED', 'SEVERITY', 'OUTCOME', 'SINCE',
              'POPULATION', 'SCALARS', 'FIXED_WORDS', 'DAY_WORDS'):
        assert env['REINA_VACC_' + c] == getattr(vac, c), c
    assert vac.DAY_WORDS == 76 and vac.FIXED_WORDS == 4928 and vac.MAX_GROUPS == txl.MAX_GROUPS and vac.PROTECTION_DAYS == 14
    macros = dict(re.findall(r'#define (REINA_VACC_\w+)\(n_days\) (.+?)(?:\s+/\*.*)?$', h, re.M))
    order = ('VACCINATIONS', 'INFECTIONS', 'COHORT', 'REPORT_WORDS')
    for n_days in (1, 365, eng.MAX_DAYS):
        fn = {}
        for name in order:
            e = macros['REINA_VACC_' + name].replace('(size_t)', '')
            e = re.sub(r'(REINA_VACC_\w+)\(n_days\)', lambda m: str(fn[m.group(1)]), e)
            fn['REINA_VACC_' + name] = eval(e, dict(n_days=n_days), env)
        assert fn['REINA_VACC_VACCINATIONS'] == vac.vaccinations_offset(n_days) and fn['REINA_VACC_INFECTIONS'] == vac.infections_offset(n_days)
        assert fn['REINA_VACC_COHORT'] == vac.cohort_offset(n_days) and fn['REINA_VACC_REPORT_WORDS'] == vac.report_words(n_days)
    enum = re.search(r'enum \{(.*?)\};', h, re.S).group(1)
    names = [re.sub(r'\s*=.*', '', x).strip() for x in re.sub(r'/\*.*?\*/', '', enum, flags=re.S).split(',')]
    names = [x for x in names if x]
    assert names[:-1] == ['REINA_VACC_S_' + s.upper() for s in vac.SCALAR_NAMES] and names[-1] == 'REINA_VACC_S_NR'


def test_library_exports_every_function_the_header_declares():
    from reina_model_amd import build
    text = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    declared = sorted(set(re.findall(r'\b(reina_[a-z_]+)\s*\(', text)))
    assert declared == sorted('reina_' + f for f in vac.VACC_FUNCTIONS)
    build.build()
    lib = eng.load_hip_library()
    for fn in declared:
        assert hasattr(lib, fn), fn
    f = vac.bind_vacc_abi(lib, 'reina_')
    assert f is not None and f['vacc_version']() == vac.VACC_VERSION == 1
    assert eng.bind_abi(lib, 'reina_')['abi_version']() == 7
    assert vac.bind_vacc_abi(par_backend.lib(), 'par_') is None
    assert os.path.join(ROOT, 'include', 'reina_vaccination.h') in build.DEPS


# ---------------------------------------------------------------------------------------------- 5. refusals (host side)

def test_refusals_on_the_host(mini_200):
    from reina_model_amd import ensemble, reports
    ctx, _ = mini_200
    for n_days in (0, eng.MAX_DAYS + 1):
        with pytest.raises(ValueError, match='n_days'):
            ctx.transmission_log.vaccination_report(n_days=n_days)
        with pytest.raises(ValueError, match='n_days'):
            vac.report_numpy(np.zeros(4, dtype=np.uint32), np.zeros(4, dtype=np.int32), np.zeros(4, dtype=np.uint32), tx_util.age_start_of(4),
                             tx_util.groups(), n_days)
    with pytest.raises(ValueError, match='age groups'):
        ctx.transmission_log.vaccination_report(age_groups=np.arange(101) // 5)          # (groups up to 20)
    v, ages = small_scenario()
    plain = _oracle(v, ages, 1)
    with pytest.raises(ValueError, match='no transmission log'):
        ensemble.vaccination_reports([plain])
    sharded = _oracle(v, ages, 1)
    sharded.n_shards = 2
    with pytest.raises(ValueError, match='sharded'):
        sharded.start_transmission_log()                                                 # (no log, so no report)

    class NoVacc:                          # an engine whose library has the log's entry points and not the report's
        vacc_f = None
    with pytest.raises(eng.EngineError, match='reina_vaccination.h'):
        reports.entry_points(NoVacc(), 'vacc_f', 'vaccination-report', 'reina_vaccination.h')

    class Log:                             # ... and its device log: the device route says so instead of falling back
        engine, members, engines, _h = NoVacc(), 1, (), None
    with pytest.raises(eng.EngineError, match='reina_vaccination.h'):
        vac.device_report_words(Log(), np.zeros(eng.MAX_AGES, dtype=np.uint8), 1, 4)
    # contexts with logs of their own are reported one by one
    reps = ensemble.vaccination_reports([ctx, ctx], n_days=30)
    assert len(reps) == 2 and reps[0] == reps[1] == ctx.transmission_log.vaccination_report(n_days=30)


# ---------------------------------------------------------------------------------------------- 6. realised protection

FLOOR_UNVACCINATED_SEVERE = 200    # severe-or-worse cases among the unvaccinated infected of the group
FLOOR_EXPECTED_SEVERE = 61         # protected infections x the unvaccinated severe share of the group


@pytest.mark.slow
def test_realised_protection_against_severe_disease_on_oracle_b():
    """300 000 agents (small_scenario scaled, care scaled with it), half of each of the decades 30-39, 40-49 and 50-59
    vaccinated in the week from day 0 (three programmes, stopped on day 7: a programme walks its window from the oldest agent
    down, so each decade keeps an unvaccinated half of the same ages), 200 days, log from day 0, seed 3, on oracle B.

    Asserted: severe_share(PROTECTED) < 0.5 x severe_share(UNVACCINATED) in every age group that reaches the count floor, and
    that at least one does.  0.5 is a condition, not a measurement: install_infection's own factor is 0.1.

    The programme stays below age 60 on purpose.  From 60 on p_death_outside_hospital is not 0, and severity_of (the
    reference's quirk Q2) then sends every symptomatic draw below that probability to FATAL whatever the factor.  The
    unvaccinated of this run have severe shares of 0.143, 0.256 and 0.626 at 60-69, 70-79 and 80+; the protected of HUS under
    a mass programme 0.022, 0.080 and 0.518: ratios near 0.15, 0.31 and 0.83, so 0.5 is no property
    of the model from 80 on.

    The floor.  With p the group's true severe share without protection, the protected draw with 0.1 p.  X_U ~ Bin(n_U, p)
    observed >= 200 means n_U p >= 145.7 at 4.5 sigma, so the observed unvaccinated share lies in [0.627 p, 1.373 p].  The
    protected share crosses half of the lowest of those when X_P >= 0.3135 m, m = n_P p; at 4.5 sigma X_P <= 0.1 m + 4.5
    sqrt(0.1 m), which stays below for m > 44.4, that is for n_P x (observed unvaccinated share) >= 44.4 x 1.373 = 61.

    Found (CPU, oracle B): 30-39: 8 996 protected infections, severe share 0.0020, against 0.0226 of 9 393 unvaccinated (212
    severe), expected 203; 40-49: 9 930, 0.0038 against 0.0324 of 9 941 (322), expected 322; 50-59: 7 086, 0.0085 against 0.0813
    of 9 223 (750), expected 576.  All three reach the floor; the realised protection is 0.91, 0.88 and 0.90."""
    n = 300000
    v, ages = small_scenario(n)
    v.update(hospital_beds=12 * n // 20000, icu_units=2 * n // 20000)
    for lo in (30, 40, 50):
        size = int(np.asarray(ages)[lo:lo + 10].sum())
        v['interventions'] = list(v['interventions']) + [['vaccinate', vu.day_date(0), size // 2, lo, lo + 9], ['vaccinate', vu.day_date(7), 0, lo, lo + 9]]
    ctx = _oracle(v, ages, 3, txlog=True)
    ctx.run(DAYS)
    r = ctx.transmission_log.vaccination_report()
    assert r.undetermined == r.bad_vacc_day == 0
    reached = []
    for g in range(r.n_groups):
        p = r.protection_against_severe(g)
        severe_u = int(r.severity[vac.UNVACCINATED, g, vac.V_SEVERE:].sum())
        expected = p.protected_count * p.unvaccinated_share if p.unvaccinated_share else 0.0
        print('group %s: protected %d share %s, unvaccinated %d share %s (severe %d), expected %.1f, protection %s' % (
            r._groups()[g], p.protected_count, p.protected_share, p.unvaccinated_count, p.unvaccinated_share, severe_u, expected, p.protection))
        if severe_u >= FLOOR_UNVACCINATED_SEVERE and expected >= FLOOR_EXPECTED_SEVERE:
            reached.append(g)
            assert p.protected_share < 0.5 * p.unvaccinated_share, (g, p)
    assert reached, 'no age group reaches the count floor'
    assert set(reached) <= {3, 4, 5}, 'the programme vaccinates the ages 30..59'
