"""Per-member disease parameters on the GPU (include/reina_params.h; reina_model_amd/parameters.py): k_group_params against the
numpy statement of the rule byte for byte, at the chunk edge of the member list, its refusals, a static and a mid-run set
against engines created with the expanded block, table rebuilds, and the particle filter that learns a multiplier."""
import copy
import ctypes
import math

import numpy as np
import pytest

import filter_util
import par_backend
from reina_model_amd import engine as eng
from reina_model_amd import ensemble, filtering, simulation
from reina_model_amd import parameters as par
from reina_model_amd.parameters import Fixed, Knob, LogNormal, ParameterSpace
from reina_model_amd.variables import VARIABLE_DEFAULTS

pytestmark = pytest.mark.gpu

EPS = float(np.float32(1.0) + np.float32(2.0 ** -23))


def _members(n, seeds, variants=None):
    """(variables, ages, setup, planner, contexts, group) of small_scenario(n), one member per seed"""
    v, ages = filter_util.small_scenario(n)
    if variants is not None:
        v['variants'] = variants
    setup = ensemble.Setup(ages, 'cuda:0', None, None, 'auto')
    planner, ctxs = setup.planner(v, seeds[0]), setup.members(v, seeds)
    group, _ = ensemble.group_for(ctxs)
    return v, ages, setup, planner, ctxs, group


def _assert_block(dev, member, want, want_pm, what=''):
    got, pm = dev.read(member)
    a = np.frombuffer(par.disease_bytes(got), dtype=np.uint32)
    b = np.frombuffer(par.disease_bytes(want), dtype=np.uint32)
    bad = np.flatnonzero(a != b)
    assert len(bad) == 0, '%s member %d: %d words of the block differ, first %d' % (what, member, len(bad), bad[0])
    assert pm.tobytes() == np.asarray(want_pm, dtype=np.float32).tobytes(), (what, member, pm, want_pm)


def _assert_carried(ctxs, before):
    for m, c in enumerate(ctxs):
        got = filter_util.carried(c.engine)
        for name, w in before[m].items():
            assert np.array_equal(got[name], w), (m, name)


KNOB_SETS_V2 = {
    'a scalar on variant 1': [Knob('inc', 'mean_incubation_duration', variants=[1])],
    'susceptibility 0-19 and 100': [Knob('kids', 'p_susceptibility', ages=(0, 19)), Knob('c', 'p_susceptibility', ages=(100, 100))],
    'susceptibility, all ages': [Knob('sus', 'p_susceptibility')],
    'a per-age field on 70-100': [Knob('old', 'p_fatal_given_critical', ages=(70, 100))],
    'a probability of variant 0': [Knob('icu', 'p_icu_death_no_beds', variants=[0])],
    'eight knobs': [Knob('beta', 'infectiousness_multiplier'), Knob('asym', 'p_asymptomatic_infection', variants=[0]),
                    Knob('inc', 'mean_incubation_duration', variants=[1]), Knob('kids', 'p_susceptibility', variants=[0], ages=(0, 19)),
                    Knob('sus1', 'p_susceptibility', variants=[1]), Knob('sym', 'p_symptomatic'),
                    Knob('sev', 'p_severe_given_symptomatic', ages=(70, 100)), Knob('out', 'p_death_outside_hospital', ages=(0, 69))],
}
KNOB_SETS_V4 = {
    'a scalar on variant 3': [Knob('rec', 'mean_duration_from_onset_to_recovery', variants=[3])],
    'susceptibility of variants 1 and 3': [Knob('s13', 'p_susceptibility', variants=[1, 3], ages=(0, 19)),
                                           Knob('s2', 'p_susceptibility', variants=[2], ages=(100, 100))],
    'eight knobs': [Knob('b%d' % k, 'infectiousness_multiplier', variants=[k]) for k in range(4)] +
                   [Knob('s%d' % k, 'p_susceptibility', variants=[k], ages=(k, 100 - k)) for k in range(4)],
}
VARIANTS_4 = [{'name': 'b1.1.7', 'infectiousness_multiplier': 1.3},
              {'name': 'p.1', 'infectiousness_multiplier': 1.6, 'mean_incubation_duration': 4.0, 'p_asymptomatic_infection': 0.5},
              {'name': 'x.3', 'infectiousness_multiplier': 0.8, 'mean_duration_from_onset_to_recovery': 9.0}]


@pytest.mark.parametrize('variants,sets', [(None, KNOB_SETS_V2), (VARIANTS_4, KNOB_SETS_V4)], ids=['V2', 'V4'])
def test_blocks_equal_the_numpy_rule_byte_for_byte(variants, sets):
    """the listed members [3, 0] get expand_numpy's block, psus_max included, for theta rows of 1, 0, a value that clamps
    (1000) and 1 + 2^-23; the unlisted members' blocks and every member's carried state are untouched"""
    import torch
    v, ages, setup, planner, ctxs, group = _members(2000, [11, 12, 13, 14, 15], variants)
    V = planner.nr_variants
    assert (planner.nr_ages, V) == (101, 2 if variants is None else 4)
    base = planner._disease
    base_pm = par.psus_max_of(base, 101, V)
    try:
        ensemble.run_group_plan(ctxs, planner.make_plan(3), group=group)   # (some state to carry)
        torch.cuda.synchronize()
        before = [filter_util.carried(c.engine) for c in ctxs]
        for what, knobs in sets.items():
            space = ParameterSpace(knobs)
            P = len(space)
            dev = par.DeviceParameters(group, base, space)
            try:
                for vals in ((1.0, 0.0), (1000.0, EPS), (0.5, 1.75)):
                    th = np.array([[vals[0] * (1 + (k % 3 == 2)) for k in range(P)], [vals[1]] * P], dtype=np.float32)
                    dev.set([3, 0], th)
                    for j, m in enumerate((3, 0)):
                        want, pm = par.expand_numpy(base, space, th[j], 101, V)
                        _assert_block(dev, m, want, pm, what)
                    for m in (1, 2, 4):
                        _assert_block(dev, m, base, base_pm, what + ' (unlisted)')
                # theta = 1 brings the base back, bit for bit (and lets the next set of knobs be made: it checks the members)
                dev.set([0, 3], np.ones((2, P), dtype=np.float32))
                for m in range(5):
                    _assert_block(dev, m, base, base_pm, what + ' (back to 1)')
            finally:
                dev.close()
        _assert_carried(ctxs, before)
    finally:
        group.close()


def test_chunk_edge():
    """the member list travels as the kernel argument, chunk(n_knobs) members a launch: chunk + 1 members, eight knobs, every
    member its own theta, every block read back"""
    space = ParameterSpace(KNOB_SETS_V2['eight knobs'])
    K = par.chunk(len(space)) + 1
    assert K == 97
    v, ages, setup, planner, ctxs, group = _members(2000, list(range(200, 200 + K)))
    base = planner._disease
    try:
        dev = par.DeviceParameters(group, base, space)
        try:
            rng = np.random.default_rng(5)
            th = rng.uniform(0.25, 2.5, size=(K, len(space))).astype(np.float32)
            order = rng.permutation(K)
            dev.set(order, th)
            for j, m in enumerate(order):
                want, pm = par.expand_numpy(base, space, th[j], 101, 2)
                _assert_block(dev, int(m), want, pm)
        finally:
            dev.close()
    finally:
        group.close()


def _raw_create(group, base, rows):
    """reina_group_params_create through the C ABI with the knob words `rows`: (return code, reina_last_error, handle)"""
    e0 = group.engines[0]
    f = e0.params_f
    knobs = (par.KnobABI * max(len(rows), 1))(*[par.KnobABI(*r) for r in rows])
    h = ctypes.c_void_p()
    rc = f['group_params_create'](group._h, ctypes.byref(base), knobs, len(rows), ctypes.byref(h))
    return rc, (e0.f['last_error']() or b'').decode(), h


def test_refusals_through_the_c_abi():
    import torch
    v, ages, setup, planner, ctxs, group = _members(2000, [21, 22, 23])
    base = planner._disease
    base_pm = par.psus_max_of(base, 101, 2)
    F = par.FIELDS.index
    try:
        e0 = group.engines[0]
        torch.cuda.synchronize()
        before = [filter_util.carried(c.engine) for c in ctxs]
        ok = (F('infectiousness_multiplier'), 3, 0, 0)
        bad_lists = {
            'n_knobs': [],
            'n_knobs ': [(F('p_susceptibility'), 1, k, k) for k in range(9)],
            'unknown field': [(len(par.FIELDS), 1, 0, 0)],
            'variant bit': [(F('infectiousness_multiplier'), 4, 0, 0)],
            'variant bit ': [(F('p_susceptibility'), 5, 0, 10)],
            'no variant': [(F('mean_incubation_duration'), 0, 0, 0)],
            'takes no variants': [(F('p_symptomatic'), 1, 0, 10)],
            'reversed or outside': [(F('p_symptomatic'), 0, 30, 20)],
            'reversed or outside ': [(F('p_susceptibility'), 1, 90, 101)],
            'takes no ages': [(F('mean_incubation_duration'), 1, 0, 5)],
            'overlap': [ok, (F('infectiousness_multiplier'), 2, 0, 0)],
            'overlap ': [(F('p_susceptibility'), 3, 0, 10), (F('p_susceptibility'), 2, 10, 20)],
            'overlap  ': [(F('p_fatal_given_critical'), 0, 0, 50), ok, (F('p_fatal_given_critical'), 0, 50, 100)],
        }
        for text, rows in bad_lists.items():
            rc, msg, h = _raw_create(group, base, rows)
            assert rc == -1, (text, rc)   # (REINA_E_INVALID)
            assert msg.startswith('reina_group_params_create') and text.strip() in msg and not h.value, (text, msg)
        # a member whose disease is not the base; a base with a probability above 1
        other = par._copy_disease(base)
        other.mean_incubation_duration[0] = other.mean_incubation_duration[0] + 1.0
        rc, msg, h = _raw_create(group, other, [ok])
        assert rc == -1 and 'reina_group_params_create' in msg and 'not the base' in msg
        # sharded members: a member that has a collective of its own
        FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int,
                              ctypes.c_void_p, ctypes.c_void_p)
        cb = FN(lambda *a: 0)
        ctxs[1].engine.set_collective(ctypes.cast(cb, ctypes.c_void_p).value, 1)
        rc, msg, h = _raw_create(group, base, [ok])
        assert rc == -1 and 'reina_group_params_create' in msg and 'sharded' in msg
        ctxs[1].engine.set_collective(None, None)
        # reina_group_params_set: checked before anything is queued
        space = ParameterSpace([Knob('beta', 'infectiousness_multiplier'), Knob('sus', 'p_susceptibility', ages=(0, 50))])
        dev = par.DeviceParameters(group, base, space)
        try:
            good = [2.0, 0.5]
            for text, members, th in (('out of range', [0, 3], [good, good]), ('listed twice', [1, 2, 1], [good] * 3),
                                      ('finite', [0, 1], [good, [-0.25, 1.0]]), ('finite', [0, 1], [good, [1.0, math.nan]]),
                                      ('finite', [2], [[math.inf, 1.0]])):
                with pytest.raises(eng.EngineError, match='reina_group_params_set.*' + text):
                    dev.set(members, np.asarray(th, dtype=np.float32))
            with pytest.raises(eng.EngineError, match='reina_group_params_read'):
                dev.read(3)
            for m in range(3):
                _assert_block(dev, m, base, base_pm, 'after the refusals')
            # (the host mirrors are untouched as well: a second handle is still made, which compares them with the base)
            par.DeviceParameters(group, base, space).close()
            dev.set([], np.zeros((0, 2), dtype=np.float32))   # (nothing to do)
        finally:
            dev.close()
        with pytest.raises(ValueError, match='nr_variants'):
            par.DeviceParameters(group, base, ParameterSpace([Knob('x', 'infectiousness_multiplier', variants=[2])]))
        other.mean_incubation_duration[0] = base.mean_incubation_duration[0]
        other.p_symptomatic[7] = 1.25
        rc, msg, h = _raw_create(group, other, [ok])
        assert rc == -1 and 'not the base' in msg    # (the members hold the base: a base above 1 can only be refused as theirs)
        _assert_carried(ctxs, before)
    finally:
        group.close()


def test_a_base_probability_above_one_is_refused():
    v, ages = filter_util.small_scenario(2000)
    one = simulation.make_context(v, age_counts=ages, seed=1, ipc=None)
    d = par._copy_disease(one._disease)
    d.p_symptomatic[7] = 1.25
    ctxs = [simulation.make_context(v, age_counts=ages, seed=s, ipc=None, disease=d) for s in (1, 2)]
    group, _ = ensemble.group_for(ctxs)
    try:
        rc, msg, h = _raw_create(group, d, [(par.FIELDS.index('infectiousness_multiplier'), 3, 0, 0)])
        assert rc == -1 and 'reina_group_params_create' in msg and 'p_symptomatic' in msg and 'outside [0, 1]' in msg
    finally:
        group.close()


SPACE3 = ParameterSpace([Knob('beta', 'infectiousness_multiplier'), Knob('old', 'p_severe_given_symptomatic', ages=(60, 100)),
                         Knob('kids', 'p_susceptibility', ages=(0, 19))])


def test_static_run_equals_engines_created_with_the_block():
    v, ages = filter_util.small_scenario(20000)
    thetas = np.array([[1.0, 1.0, 1.0], [1.5, 0.5, 0.25], [0.7, 3.0, 2.0], [EPS, 1000.0, 0.0]], dtype=np.float32)
    seeds = [61, 62, 63, 64]
    hist, ctxs = ensemble.run_parameter_ensemble(v, thetas, seeds, 60, SPACE3, age_counts=ages)
    base = simulation.make_context(v, age_counts=ages, seed=1, ipc=None)._disease
    for m, (sd, th) in enumerate(zip(seeds, thetas)):
        block, _ = par.expand_numpy(base, SPACE3, th, 101, 2)
        assert par.disease_bytes(ctxs[m]._disease) == par.disease_bytes(block)
        one = simulation.make_context(v, age_counts=ages, seed=sd, ipc='auto', disease=block)
        assert np.array_equal(one.run(60), hist[m]), m
    inf = filter_util.totals(hist, 'all_infected')[:, -1]
    assert len(set(inf.tolist())) >= 3, inf


def test_mid_run_set_equals_a_clone_into_an_engine_created_with_the_block():
    """A runs 25 days under the base, is set theta', runs 25 more; the reference is built of reina_create and the clone only:
    [C, B], C as A, B created with expand_numpy(base, theta'), 25 days, B <- C, 25 more days"""
    v, ages, setup, planner, ctxs, group = _members(20000, [71, 72])
    base = planner._disease
    th = np.array([1.5, 0.5, 0.25], dtype=np.float32)
    try:
        dev = par.DeviceParameters(group, base, SPACE3)
        try:
            ensemble.run_group_plan(ctxs, planner.make_plan(25), group=group)
            dev.set([0], th[None])
            got = ensemble.run_group_plan(ctxs, planner.make_plan(25), group=group)
        finally:
            dev.close()
        planner2 = setup.planner(v, 71)
        block, _ = par.expand_numpy(base, SPACE3, th, 101, 2)
        ref = [setup.context(v, 71), setup.context(v, 71, disease=block)]
        rgroup, _ = ensemble.group_for(ref)
        try:
            ensemble.run_group_plan(ref, planner2.make_plan(25), group=rgroup)
            filtering.clone_group(rgroup, [(1, 0)])
            want = ensemble.run_group_plan(ref, planner2.make_plan(25), group=rgroup)
        finally:
            rgroup.close()
        assert np.array_equal(got[0], want[1])
        assert not np.array_equal(got[0], want[0])      # (theta' changed the run)
        assert filter_util.totals(got, 'all_infected')[0, -1] > 0
        filter_util.assert_same_day_state(ctxs[0], ref[1])
    finally:
        group.close()


def test_setting_the_same_theta_again_changes_nothing_and_table_rebuilds_keep_the_block():
    """days 0-49 of the default scenario cross its dated limit-mobility rebuilds (days 23 and 26): member 0's whole parameter
    block is uploaded again from its host mirror there"""
    th = np.array([[1.4, 0.5, 0.5], [0.8, 2.0, 1.5]], dtype=np.float32)
    runs = []
    for again in (True, False):
        v, ages, setup, planner, ctxs, group = _members(20000, [81, 82])
        base = planner._disease
        try:
            dev = par.DeviceParameters(group, base, SPACE3)
            try:
                dev.set([0, 1], th)
                if again:
                    h1 = ensemble.run_group_plan(ctxs, planner.make_plan(20), group=group)
                    dev.set([1, 0], th[::-1])
                    h2 = ensemble.run_group_plan(ctxs, planner.make_plan(30), group=group)
                    runs.append(np.concatenate([h1, h2], axis=1))
                else:
                    runs.append(ensemble.run_group_plan(ctxs, planner.make_plan(50), group=group))
                for m in range(2):
                    want, pm = par.expand_numpy(base, SPACE3, th[m], 101, 2)
                    _assert_block(dev, m, want, pm, 'after the rebuilds')
            finally:
                dev.close()
        finally:
            group.close()
    assert np.array_equal(runs[0], runs[1])
    assert filter_util.totals(runs[0], 'all_infected')[:, -1].min() > 0


@pytest.fixture(scope='module')
def small_observations():
    v, ages = filter_util.small_scenario(20000)
    truth = simulation.make_context(v, age_counts=ages, seed=777, ipc='auto', engine_factory=par_backend.par_engine_factory)
    obs = filter_util.observations(truth.run(90), v['start_date'], range(10, 90))
    return v, ages, dict(observations=obs, obs_model=filtering.ObservationModel({'all_detected': 8.0, 'in_ward': 8.0}), window=7,
                         days=90, seeds=list(range(100, 108)), filter_seed=5, age_counts=ages)


ONES = ParameterSpace([Knob('beta', 'infectiousness_multiplier', prior=Fixed(1.0)), Knob('sus', 'p_susceptibility', prior=Fixed(1.0)),
                       Knob('sev', 'p_severe_given_symptomatic', ages=(50, 100), prior=Fixed(1.0))])


@pytest.mark.parametrize('txlog', [False, True], ids=['unlogged', 'logged'])
def test_filter_with_fixed_ones_equals_the_filter_without_parameters(small_observations, txlog):
    v, ages, kw = small_observations
    a = filtering.particle_filter(v, 8, txlog=txlog, **kw)
    b = filtering.particle_filter(v, 8, txlog=txlog, parameters=ONES, **kw)
    try:
        assert sum(w['resampled'] for w in a.windows) >= 2
        assert np.array_equal(a.ancestors, b.ancestors) and np.array_equal(a.ess, b.ess)
        assert np.array_equal(a.loglik, b.loglik) and a.log_evidence == b.log_evidence
        assert np.array_equal(a.paths(), b.paths())
        assert np.all(b.parameters == 1.0) and b.parameters.shape == (8, 3)
        assert all(np.all(w['theta'] == 1.0) and abs(w['weights'].sum() - 1) < 1e-12 for w in b.windows)
        if txlog:
            for x, y in zip(a.log_reports(), b.log_reports()):
                assert np.array_equal(x.incidence, y.incidence)
    finally:
        a.close()
        b.close()


THETA_STAR = 1.2
# RATIO_MEASURED: the width of the final weighted 5-95 % band of beta over the width of the prior's, as the first run on an
# MI355X gave it.  The run is seeded and the engine deterministic, so the margin is not for noise: it is room for a later
# change that realises the same posterior with other draws.  A 5-95 % band read off n weighted particles has a relative
# standard deviation of about 0.91 / sqrt(n) (two normal quantiles at +-1.645 sigma, sd 2.11 sigma / sqrt(n) each, over a width
# of 3.29 sigma); with n = K / 2 = 64 (the resampling threshold keeps the ESS there) that is 11 %, and the margin is two of them.
RATIO_MEASURED = 0.0162   # (band [1.1846, 1.2012] around theta* = 1.2, prior band [0.611, 1.638]; 4 resamples)
RATIO_MARGIN = 0.25


@pytest.fixture(scope='module')
def twin():
    """truth: seed 10007 of the default scenario on HUS under infectiousness_multiplier x THETA_STAR; observed: all_detected and
    in_ward on days 30-150; K = 128, the prior LogNormal(1, 0.3)"""
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    space = ParameterSpace([Knob('beta', 'infectiousness_multiplier', prior=LogNormal(1.0, 0.3), bounds=(0.25, 4.0))])
    plain = simulation.make_context(v, seed=10007, ipc='auto')
    block, _ = par.expand_numpy(plain._disease, space, [THETA_STAR], plain.nr_ages, plain.nr_variants)
    truth = simulation.make_context(v, seed=10007, ipc='auto', disease=block)
    obs = filter_util.observations(truth.run(151), v['start_date'], range(30, 151))
    K = 128
    r = filtering.particle_filter(v, K, observations=obs, obs_model=filtering.ObservationModel({'all_detected': 10.0, 'in_ward': 10.0}),
                                  window=7, days=151, seeds=list(range(1, K + 1)), filter_seed=1, parameters=space)
    yield space, r
    r.close()


def test_twin_experiment_recovers_the_multiplier(twin):
    space, r = twin
    band = r.parameter_band('beta', (0.05, 0.5, 0.95))
    lo, mid, hi = band.iloc[-1].tolist()
    prior = space.knobs[0].prior
    ratio = (hi - lo) / (prior.quantile(0.95) - prior.quantile(0.05))
    print('twin: theta* %.3f, final band [%.4f, %.4f, %.4f], mean %.4f, width ratio to the prior %.4f, resamples %d, log evidence %.2f'
          % (THETA_STAR, lo, mid, hi, r.parameter_mean('beta').iloc[-1], ratio, sum(w['resampled'] for w in r.windows), r.log_evidence))
    assert len(band) == len(r.windows) and r.parameters.shape == (128, 1)
    assert lo <= THETA_STAR <= hi
    assert ratio < 1.0
    assert ratio < RATIO_MEASURED * (1.0 + RATIO_MARGIN)


def test_forecast_continues_under_the_final_theta(twin):
    space, r = twin
    n0 = len(r.windows)
    final = r.parameters.copy()
    hist = r.forecast(30)
    assert hist.shape[:2] == (128, 30) and len(r.windows) == n0 + 1 and np.array_equal(r.windows[-1]['theta'], final)
    dev = r.device_parameters
    for m in range(128):
        want, pm = dev.expand(final[m])
        _assert_block(dev, m, want, pm, 'after the forecast')
        assert par.disease_bytes(r.contexts[m]._disease) == par.disease_bytes(want)
    assert len(np.unique(final)) > 16
