"""A policy and a log in one run, and the regime report, on oracle B (reina_model_amd/policy.py, regime.py; DESIGN.md section
6q): the host-driven logged policy run against the two routes it joins, a run in stretches, the report's specification against
a plain per-agent walker, its ties to the log report, and the refusals.  The inputs are those of tests/regime_util.py; this
module also asserts that they exercise what tests/test_regime_gpu.py needs."""
import functools

import numpy as np
import pytest

import policy_util as pu
import regime_util as ru
from par_backend import par_engine_factory
from reina_model_amd import engine as eng
from reina_model_amd import ensemble, filtering, policy as pol, regime as rgm, simulation, txlog as txl


def _oracle(seed=1, policy=None, interventions=None, ages=None):
    v, mini_ages = ru.scenario()
    return pu.make(v, mini_ages if ages is None else ages, seed=seed, factory=par_engine_factory, policy=policy, interventions=interventions)


@functools.lru_cache(maxsize=None)
def _run(seed):
    """DAYS days of seed `seed` under the regime policy with both logs from day 0, in one piece"""
    c = _oracle(seed, ru.regime_policy())
    c.start_course_log()
    assert not c.transmission_log.on_device and c.engine.regime_f is None and c.engine.policy_f is None
    hist = c.run(ru.DAYS)
    return c, hist


def _words(c):
    return c.transmission_log.words(), c.course_log.words()


# ---------------------------------------------------------------------------------------------- 0. the inputs do what the GPU tests need

def test_the_inputs_switch_and_cross():
    firsts = []
    for seed, infected in zip(ru.SEEDS, (2242, 2519, 2653)):
        c, _ = _run(seed)
        up, down = pu.switches(c.policy_levels)
        assert sorted(set(c.policy_levels.tolist())) == [0, 1, 2], seed
        assert len(up) >= 2 and len(down) >= 1, (seed, up, down)
        firsts.append((int(up[0]), int(down[0])))
        rep = c.transmission_log.regime_report()
        assert rep.infected == infected and rep.unlabelled == 0 and rep.in_range == rep.dated
        assert (rep.infections[:3].sum(axis=(1, 2)) > 0).all(), 'every level holds infections'
        assert int((rep.crossing[:3, :3] > 0).sum()) >= 6 and rep.links_crossing > 0
        assert np.array_equal(c.policy_level_by_day[:ru.DAYS], c.policy_levels) and (c.policy_level_by_day[ru.DAYS:] == -1).all()
    assert len({up for up, _ in firsts}) > 1 and len({down for _, down in firsts}) > 1, 'the members switch on the same days: %s' % (firsts,)


# ---------------------------------------------------------------------------------------------- 1. the host-driven route is the two it joins

def test_never_policy_records_what_the_log_route_records():
    a = _oracle(1)
    a.start_course_log()
    ha = pol.run_host_driven(a, pu.never_policy(), 80)
    b = _oracle(1)
    b.start_course_log()
    hb = txl.run_host_driven(b, 80)
    assert np.array_equal(ha, hb)
    for x, y, what in zip(_words(a), _words(b), ('log', 'course')):
        ru.assert_words(x, y, what)
    assert int((a.transmission_log.words() & 0xFFFF < txl.BEFORE).sum()) > 100
    assert not a.policy_levels.any() and (a.policy_level_by_day[:80] == 0).all()


def test_forced_policy_records_the_log_of_the_dated_intervention():
    ivs = [iv for iv in pu.hus_variables()['interventions'] if not (iv[0] == 'limit-mobility' and len(iv) == 3)]
    date, day, days = '2020-06-10', 113, 160
    a = _oracle(1, interventions=ivs)
    a.start_course_log()
    ha = pol.run_host_driven(a, pu.forced_policy(date), days)
    b = _oracle(1, interventions=ivs + [['limit-mobility', date, 30]])
    b.start_course_log()
    hb = b.run(days)
    assert list(a.policy_levels) == [0] * day + [1] * (days - day)
    assert np.array_equal(ha, hb)
    for x, y, what in zip(_words(a), _words(b), ('log', 'course')):
        ru.assert_words(x, y, what)
    c = _oracle(1, interventions=ivs)
    c.start_transmission_log()
    c.run(days)
    assert not np.array_equal(c.transmission_log.words(), b.transmission_log.words()), 'the intervention changes nothing'


def test_the_logs_observe_and_never_steer():
    logged, hl = _run(1)
    plain = _oracle(1, ru.regime_policy())
    hp = plain.run(ru.DAYS)
    pu.assert_same_run(logged, plain, hl, hp, planes=False)


# ---------------------------------------------------------------------------------------------- 2. a run in stretches

def test_stretches_accumulate():
    whole, hist = _run(1)
    parts = _oracle(1, ru.regime_policy())
    parts.start_course_log()
    hs = [parts.run(n) for n in ru.STRETCHES]
    assert np.array_equal(np.concatenate(hs), hist)
    for x, y, what in zip(_words(parts), _words(whole), ('log', 'course')):
        ru.assert_words(x, y, what)
    assert np.array_equal(parts.policy_level_by_day, whole.policy_level_by_day)
    assert len(parts.policy_levels) == ru.STRETCHES[-1], 'policy_levels keeps its meaning: the last run'
    assert parts.transmission_log.regime_report() == whole.transmission_log.regime_report()


def test_iterate_records_on_a_policy_context():
    c = _oracle(1, ru.regime_policy())
    c.start_transmission_log()
    for _ in range(30):
        c.iterate()
    d = _oracle(1)
    d.start_transmission_log()
    d.run(30)
    ru.assert_words(c.transmission_log.words(), d.transmission_log.words(), 'log')


# ---------------------------------------------------------------------------------------------- 3. the specification against the walker

def _late():
    c = _oracle(1, ru.regime_policy())
    c.run(ru.LATE_LOG_DAY)
    c.start_course_log()
    c.run(ru.DAYS - ru.LATE_LOG_DAY)
    return c


@pytest.mark.parametrize('name', sorted(ru.labellings(np.zeros(ru.DAYS))))
def test_report_numpy_is_the_walker(name):
    c, _ = _run(1)
    labels, n_days = ru.labellings(c.policy_levels)[name]
    rep = ru.spec_report(c, labels, n_days)
    want = ru.walk_report(*ru.state(c), c.age_start, c._tx_groups(None)[0], labels, n_days)
    ru.assert_words(rep.words, want, name)
    assert int(rep.days.sum()) == n_days and int(rep.crossing.sum()) == rep.links == int(rep.link_phase.sum())
    if name == 'fifth':
        assert rep.unlabelled > 0 and int(rep.days[8]) == ru.DAYS // 5
    if name == 'n_days_1':
        assert rep.in_range < rep.dated and int(rep.infections[8].sum()) > 0


def test_report_numpy_is_the_walker_for_a_log_begun_mid_run():
    c = _late()
    labels = rgm.policy_labels(c, ru.DAYS)
    assert (c.policy_level_by_day[:ru.DAYS] >= 0).all(), 'the levels of both stretches'
    rep = c.transmission_log.regime_report()
    want = ru.walk_report(*ru.state(c), c.age_start, c._tx_groups(None)[0], labels, ru.DAYS)
    ru.assert_words(rep.words, want, 'late log')
    assert rep.dated < rep.infected and int(rep.crossing[8].sum()) > 0, 'infectors from before the log began'


# ---------------------------------------------------------------------------------------------- 4. ties to the log report

@pytest.mark.parametrize('name', ['levels', 'fifth', 'modulo'])
def test_ties_to_the_log_report(name):
    c, _ = _run(2)
    n_days = ru.DAYS + 40
    lab, _ = ru.labellings(c.policy_levels)[name]
    labels = np.full(n_days, rgm.NO_REGIME, dtype=np.uint8)
    labels[:ru.DAYS] = lab
    ru.assert_ties(c.transmission_log.regime_report(labels, n_days=n_days), c.transmission_log.report(n_days=n_days))


def test_accessors():
    c, _ = _run(3)
    rep = c.transmission_log.regime_report()
    log = c.transmission_log.report()
    rn = rep.reproduction_number()
    assert list(rn.index) == list(rgm.SLOT_NAMES) and int(rn['cohort'].sum()) == rep.infected and int(rn['days'].sum()) == ru.DAYS
    assert rn['r_c'].iloc[0] == int(rep.cohort[0, :, 1].sum()) / int(rep.cohort[0, :, 0].sum())
    assert rep.generation_interval().total() == log.generation_interval().total() == sum(rep.generation_interval(r).total() for r in range(8)) + \
        rep.generation_interval('none').total()
    assert rep.serial_interval().mean() == log.serial_interval().mean()
    assert rep.onset_to_transmission(1).total() == int(rep.tost[1].sum())
    share = rep.presymptomatic_share()
    assert share.iloc[1] == int(rep.link_phase[1, 0]) / int(rep.link_phase[1, :2].sum())
    assert int(rep.mixing_frame().values.sum()) == rep.links and int(rep.mixing_frame(2).values.sum()) == int(rep.mixing[2].sum())
    assert int(rep.crossing_frame().values.sum()) == rep.links
    assert int(rep.infections_frame().values.sum()) == rep.infected
    off = rep.offspring(0)
    k = np.arange(rgm.OFFSPRING_BINS)
    mean = float((off.counts * k).sum()) / off.cases
    var = float((off.counts * k * k).sum()) / off.cases - mean * mean
    assert off.cases == int(rep.cohort[0, :, 2].sum()) and abs(off.mean - mean) < 1e-12
    assert (off.dispersion_k is None) == (var <= mean) and (off.dispersion_k is None or abs(off.dispersion_k - mean * mean / (var - mean)) < 1e-9)
    assert rep.offspring('none').cases == 0 and rep.offspring('none').mean is None
    with pytest.raises(ValueError):
        rep.offspring(9)


# ---------------------------------------------------------------------------------------------- 5. validation and refusals

def test_labels_and_n_days_are_validated():
    c, _ = _run(1)
    log = c.transmission_log
    good = np.zeros(ru.DAYS, dtype=np.uint8)
    for bad in (np.full(ru.DAYS, 8), np.full(ru.DAYS, -1), np.zeros(ru.DAYS - 1, dtype=np.uint8), np.zeros(ru.DAYS), np.zeros((2, ru.DAYS), dtype=np.uint8)):
        with pytest.raises(ValueError, match='label'):
            log.regime_report(bad)
    for n_days in (0, eng.MAX_DAYS + 1):
        with pytest.raises(ValueError, match='n_days'):
            log.regime_report(good, n_days=n_days)
    assert log.regime_report(np.zeros(ru.DAYS + 5, dtype=np.int64)).n_days == ru.DAYS, 'labels beyond n_days are not looked at'
    plain = _oracle(1)
    plain.start_transmission_log()
    plain.run(10)
    with pytest.raises(ValueError, match='never ran under a policy'):
        plain.transmission_log.regime_report()
    with pytest.raises(ValueError, match='keeps no transmission log'):
        ensemble.regime_reports([_oracle(1)])
    with pytest.raises(ValueError, match='one sequence of labels per context'):
        ensemble.regime_reports([c], labels=[good, good])


def test_labels_by_value_labels_a_dated_run():
    labels, values = rgm.labels_by_value([1.0, 1.0, 0.5, 0.5, 1.0, 0.7])
    assert labels.tolist() == [0, 0, 1, 1, 0, 2] and values == [1.0, 0.5, 0.7] and labels.dtype == np.uint8
    assert rgm.labels_by_value(range(8))[0].tolist() == list(range(8))
    with pytest.raises(ValueError, match='more than 8'):
        rgm.labels_by_value(range(9))
    c = _oracle(1)
    c.start_transmission_log()
    c.run(ru.DAYS)
    labels, values = rgm.labels_by_value(c.mobility_history)
    assert len(values) >= 2
    rep = c.transmission_log.regime_report(labels)
    assert int(rep.days.sum()) == ru.DAYS and rep.unlabelled == 0 and int((rep.days[:8] > 0).sum()) == len(values)
    ru.assert_words(rep.words, ru.walk_report(*ru.state(c), c.age_start, c._tx_groups(None)[0], labels, ru.DAYS), 'dated run')


def test_group_reports_take_every_members_own_labels():
    ctxs = [_run(s)[0] for s in ru.SEEDS]
    reps = ensemble.regime_reports(ctxs)
    for c, r in zip(ctxs, reps):
        assert r == c.transmission_log.regime_report() and np.array_equal(r.labels, c.policy_levels)
    assert len({r.words.tobytes() for r in reps}) == len(ru.SEEDS)


def test_policy_ensemble_keeps_logs_on_the_host_driven_route():
    v, ages = ru.scenario()
    hist, levels, ctxs = ensemble.run_policy_ensemble(v, ru.SEEDS[:2], ru.DAYS, ru.regime_policy(), age_counts=ages, engine_factory=par_engine_factory,
                                                      course=True)
    for m, seed in enumerate(ru.SEEDS[:2]):
        solo, hs = _run(seed)
        assert np.array_equal(hist[m], hs) and np.array_equal(levels[m], solo.policy_levels)
        for x, y, what in zip(_words(ctxs[m]), _words(solo), ('log', 'course')):
            ru.assert_words(x, y, '%s of member %d' % (what, m))


def test_the_refusals_that_remain():
    v, ages = ru.scenario()
    p = ru.regime_policy()
    c, _ = _run(1)
    with pytest.raises(ValueError, match='policy|transmission log'):
        c.snapshot()
    sharded = _oracle(1, p)
    sharded.n_shards = 2
    with pytest.raises(ValueError, match='sharded'):
        sharded.start_transmission_log()
    with pytest.raises(ValueError, match='sharded'):
        pol.run_host_driven(sharded, p, 1)
    with pytest.raises(ValueError, match='a policy is refused'):
        filtering.particle_filter(v, 4, days=7, age_counts=ages, engine_factory=par_engine_factory, policy=p)
    planner = _oracle(1)
    plan = planner.make_plan(5, policy=p)
    members = [_oracle(1), _oracle(2)]
    with pytest.raises(ValueError, match='member_plans'):
        ensemble.run_group_plan(members, plan, member_plans=[plan, plan], policy=p, txlog=True)
    assert all(m.transmission_log is None and m.day == 0 for m in members)
    # the keywords of the constructor ask for the library's combined run: a library without it refuses them as it always has
    with pytest.raises(ValueError, match='policy'):
        simulation.make_context(v, age_counts=ages, seed=1, engine_factory=par_engine_factory, policy=p, course=True)
    # a log on the device cannot be recorded by the host-driven route, and the other way round
    class OnDevice:
        on_device = True
    fake = _oracle(1, p)
    fake.transmission_log = OnDevice()
    with pytest.raises(ValueError, match='on the device'):
        pol.run_host_driven(fake, p, 1)
    host = _oracle(1, p)
    host.start_transmission_log()
    with pytest.raises(ValueError, match='host'):
        host.run_plan(_oracle(1).make_plan(3, policy=p))


def test_a_library_with_the_log_but_without_the_combined_run(monkeypatch):
    """a policy Context keeps its log in host memory there, and a group refuses the combination before anything is created"""
    p = ru.regime_policy()
    monkeypatch.setattr(eng, 'is_device', lambda engine: True)
    c = _oracle(1, p)
    c.engine.txlog_f = {'txlog_create': None}   # (never called: the log must not go to the device)
    assert c.engine.regime_f is None
    c.start_transmission_log()
    assert not c.transmission_log.on_device
    monkeypatch.undo()
    members = [_oracle(1), _oracle(2)]
    plan = _oracle(1).make_plan(5, policy=p)
    with pytest.raises(ValueError, match='cannot be combined on this engine library'):
        ensemble.run_group_plan(members, plan, policy=p, txlog=True)
    assert all(m.transmission_log is None and m.day == 0 for m in members)
