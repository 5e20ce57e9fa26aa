"""Per-member disease parameters on the CPU (reina_model_amd/parameters.py; include/reina_params.h): the numpy statement of the
expansion rule, what a ParameterSpace refuses, the Liu-West step, the filter's refusal on a library without the entry points,
and run_parameter_ensemble on oracle B against single Contexts handed the same expanded block."""
import ctypes
import math

import numpy as np
import pytest

import filter_util
import par_backend
from reina_model_amd import engine as eng
from reina_model_amd import ensemble, filtering, simulation
from reina_model_amd import parameters as par
from reina_model_amd.parameters import Fixed, Knob, LogNormal, ParameterSpace, Uniform

PAR = par_backend.par_engine_factory
A, V = 101, 2


@pytest.fixture(scope='module')
def base():
    """the default scenario's disease block (ages 0..100, wild-type and one variant)"""
    v, ages = filter_util.small_scenario(2000)
    c = simulation.make_context(v, age_counts=ages, seed=1, ipc=None, engine_factory=PAR)
    assert (c.nr_ages, c.nr_variants) == (A, V)
    return c._disease


def _arr(d, name):
    return np.ctypeslib.as_array(getattr(d, name)).copy()


def _same_outside(d, b, touched):
    """every field of the block but `touched` is the base's, byte for byte"""
    for name, _ in eng.Disease._fields_:
        if name not in touched:
            x, y = getattr(d, name), getattr(b, name)
            if hasattr(x, '__len__'):
                assert ctypes.string_at(x, ctypes.sizeof(x)) == ctypes.string_at(y, ctypes.sizeof(y)), name
            else:
                assert x == y, name


def test_theta_one_is_the_base(base):
    space = ParameterSpace([Knob('beta', 'infectiousness_multiplier'), Knob('sus', 'p_susceptibility'),
                            Knob('sev', 'p_severe_given_symptomatic', ages=(70, 100)), Knob('inc', 'mean_incubation_duration', variants=[1])])
    d, pm = par.expand_numpy(base, space, [1, 1, 1, 1], A, V)
    assert par.disease_bytes(d) == par.disease_bytes(base)
    # reina_create's psus_max: per variant the maximum over a < nr_ages from 0.0f, zero for the variants beyond
    sus = _arr(base, 'p_susceptibility')
    want = np.zeros(eng.MAX_VARIANTS, dtype=np.float32)
    want[:V] = sus[:V, :A].max(axis=1)
    assert pm.dtype == np.float32 and pm.tobytes() == want.tobytes() and np.all(want[:V] > 0)


def test_scaling_clamp_and_zero(base):
    space = ParameterSpace([Knob('beta', 'infectiousness_multiplier'), Knob('asym', 'p_asymptomatic_infection')])
    b_im, b_pa = _arr(base, 'infectiousness_multiplier'), _arr(base, 'p_asymptomatic_infection')
    t = np.float32(1.0) + np.float32(2.0 ** -23)
    d, _ = par.expand_numpy(base, space, [t, 1000.0], A, V)
    assert _arr(d, 'infectiousness_multiplier')[:V].tobytes() == (b_im[:V] * t).astype(np.float32).tobytes()   # one float32 product
    assert np.all(_arr(d, 'infectiousness_multiplier')[V:] == b_im[V:])
    assert np.all(b_pa[:V] > 0) and np.all(_arr(d, 'p_asymptomatic_infection')[:V] == np.float32(1.0))       # the clamp holds at 1
    d, _ = par.expand_numpy(base, space, [1000.0, 0.0], A, V)
    assert np.all(_arr(d, 'infectiousness_multiplier')[:V] == b_im[:V] * np.float32(1000.0))                  # no clamp: not a p_ field
    assert np.all(_arr(d, 'p_asymptomatic_infection') == 0)                                                    # theta = 0 applies
    _same_outside(d, base, ('infectiousness_multiplier', 'p_asymptomatic_infection'))


def test_age_band_and_variant_mask(base):
    space = ParameterSpace([Knob('old', 'p_fatal_given_critical', ages=(70, 100)), Knob('v1', 'mean_incubation_duration', variants=[1]),
                            Knob('kids', 'p_susceptibility', variants=[1], ages=(0, 19))])
    d, _ = par.expand_numpy(base, space, [0.5, 2.0, 0.25], A, V)
    f0, f1 = _arr(base, 'p_fatal_given_critical'), _arr(d, 'p_fatal_given_critical')
    assert np.array_equal(f1[:70], f0[:70]) and np.array_equal(f1[101:], f0[101:])
    assert np.array_equal(f1[70:101], f0[70:101] * np.float32(0.5)) and np.any(f0[70:101] > 0)
    i0, i1 = _arr(base, 'mean_incubation_duration'), _arr(d, 'mean_incubation_duration')
    assert i1[0] == i0[0] and i1[1] == i0[1] * np.float32(2.0) and np.array_equal(i1[2:], i0[2:])
    s0, s1 = _arr(base, 'p_susceptibility'), _arr(d, 'p_susceptibility')
    assert np.array_equal(s1[0], s0[0]) and np.array_equal(s1[1, 20:], s0[1, 20:])
    assert np.array_equal(s1[1, :20], s0[1, :20] * np.float32(0.25))
    _same_outside(d, base, ('p_fatal_given_critical', 'mean_incubation_duration', 'p_susceptibility'))


def test_psus_max_follows_the_scaled_band(base):
    b = par._copy_disease(base)
    for v in range(V):
        for a in range(A):
            b.p_susceptibility[v][a] = 0.5 if a < 50 else 0.25   # the maximum sits in ages 0-49
    young = ParameterSpace([Knob('young', 'p_susceptibility', variants=[0], ages=(0, 49))])
    _, pm = par.expand_numpy(b, young, [0.25], A, V)              # the maximum leaves the scaled band: now 0.25, held by 50+
    assert pm.tolist() == [0.25, 0.5, 0.0, 0.0]
    _, pm = par.expand_numpy(b, young, [1.5], A, V)
    assert pm.tolist() == [0.75, 0.5, 0.0, 0.0]
    old = ParameterSpace([Knob('old', 'p_susceptibility', ages=(100, 100))])
    _, pm = par.expand_numpy(b, old, [3.0], A, V)                 # the maximum enters the scaled band: age 100 alone, 0.75
    assert pm.tolist() == [0.75, 0.75, 0.0, 0.0]
    _, pm = par.expand_numpy(b, old, [8.0], A, V)                 # ... a relative susceptibility: scaled, not clamped
    assert pm.tolist() == [2.0, 2.0, 0.0, 0.0]
    # the default scenario's own reaches above 1, and theta = 1 keeps it (test_theta_one_is_the_base)
    assert par.CLAMPED == ('p_asymptomatic_infection', 'p_hospital_death_no_beds', 'p_icu_death_no_beds', 'p_symptomatic',
                           'p_severe_given_symptomatic', 'p_critical_given_severe', 'p_fatal_given_critical', 'p_death_outside_hospital')


def test_the_space_refuses_what_the_abi_refuses(base):
    ok = Knob('beta', 'infectiousness_multiplier')
    with pytest.raises(ValueError):
        ParameterSpace([])
    with pytest.raises(ValueError):
        ParameterSpace([Knob('k%d' % k, 'p_susceptibility', ages=(k, k)) for k in range(9)])
    with pytest.raises(ValueError, match='unknown field'):
        ParameterSpace([Knob('x', 'infectiousness_over_time')])
    with pytest.raises(ValueError, match='unknown field'):
        ParameterSpace([Knob('x', 'p_mask_protects_others')])
    with pytest.raises(ValueError, match='no variants'):
        ParameterSpace([Knob('x', 'p_symptomatic', variants=[0])])
    with pytest.raises(ValueError, match='no ages'):
        ParameterSpace([Knob('x', 'mean_incubation_duration', ages=(0, 10))])
    with pytest.raises(ValueError, match='reversed'):
        ParameterSpace([Knob('x', 'p_symptomatic', ages=(30, 20))])
    with pytest.raises(ValueError, match='at least one'):
        ParameterSpace([Knob('x', 'p_susceptibility', variants=[])])
    for a, b in ((ok, Knob('again', 'infectiousness_multiplier', variants=[1])),
                 (Knob('a', 'p_symptomatic', ages=(0, 50)), Knob('b', 'p_symptomatic', ages=(50, 100))),
                 (Knob('a', 'p_susceptibility', variants=[0, 1], ages=(0, 10)), Knob('b', 'p_susceptibility', variants=[1], ages=(10, 20)))):
        with pytest.raises(ValueError, match='overlap'):
            ParameterSpace([a, b])
    # neighbours that share no cell are taken
    ParameterSpace([Knob('a', 'p_susceptibility', variants=[0], ages=(0, 10)), Knob('b', 'p_susceptibility', variants=[1], ages=(0, 10)),
                    Knob('c', 'p_susceptibility', variants=[0], ages=(11, 20)), Knob('d', 'p_symptomatic'), ok])
    # what needs the population
    with pytest.raises(ValueError, match='nr_ages'):
        par.expand_numpy(base, ParameterSpace([Knob('x', 'p_symptomatic', ages=(90, 101))]), [1.0], A, V)
    with pytest.raises(ValueError, match='nr_variants'):
        par.expand_numpy(base, ParameterSpace([Knob('x', 'infectiousness_multiplier', variants=[2])]), [1.0], A, V)
    for bad in (-0.5, math.nan, math.inf):
        with pytest.raises(ValueError, match='finite'):
            par.expand_numpy(base, ParameterSpace([ok]), [bad], A, V)
    with pytest.raises(ValueError, match='one theta per knob'):
        par.expand_numpy(base, ParameterSpace([ok]), [1.0, 1.0], A, V)
    b = par._copy_disease(base)
    b.p_symptomatic[3] = 1.5
    with pytest.raises(ValueError, match='outside'):
        par.expand_numpy(b, ParameterSpace([ok]), [1.0], A, V)
    with pytest.raises(ValueError):
        Knob('x', 'p_symptomatic', prior=LogNormal(1, 0.3), bounds=(0.0, 2.0))
    with pytest.raises(ValueError):
        Knob('x', 'p_symptomatic', prior=0.5)


def _space3():
    return ParameterSpace([Knob('beta', 'infectiousness_multiplier', prior=LogNormal(1.0, 0.3), bounds=(0.25, 4.0)),
                           Knob('hosp', 'p_severe_given_symptomatic', prior=Uniform(0.5, 1.5), bounds=(0.5, 1.5)),
                           Knob('fix', 'p_symptomatic', prior=Fixed(0.75))])


def _particles(K, seed):
    space = _space3()
    gen = np.random.Generator(np.random.PCG64(np.random.SeedSequence([seed, 1])))
    lt = space.draw_prior(K, gen)
    rng = np.random.default_rng(seed)
    w = rng.random(K) ** 3
    w /= w.sum()
    anc, _ = filtering.assign_in_place(filtering.systematic_offspring(w, 0.37))
    return space, gen, lt, w, anc


def test_prior_draws():
    space, _, lt, _, _ = _particles(4000, 3)
    th = space.theta_of(lt)
    assert th.shape == (4000, 3) and np.all(th[:, 2] == np.float64(np.float32(0.75)))
    assert np.all((th[:, 0] >= 0.25) & (th[:, 0] <= 4.0)) and np.all((th[:, 1] >= 0.5) & (th[:, 1] <= 1.5))
    # (4000 draws: the median of a LogNormal(1, 0.3) within 4.5 sigma of its sample median's spread, 1.2533 * 0.3 / sqrt(4000))
    assert abs(np.log(np.median(th[:, 0]))) < 4.5 * 1.2533 * 0.3 / math.sqrt(4000)
    assert abs(th[:, 1].mean() - 1.0) < 4.5 * (1.0 / math.sqrt(12)) / math.sqrt(4000)
    # reproducible for a seed, and another seed draws another table
    assert np.array_equal(lt, _particles(4000, 3)[2]) and not np.array_equal(lt, _particles(4000, 4)[2])
    # without a Uniform prior the table is K x P standard normals in C order
    s2 = ParameterSpace([Knob('a', 'infectiousness_multiplier', prior=LogNormal(2.0, 0.5), bounds=(1e-6, 1e6)), Knob('b', 'p_symptomatic')])
    z = np.random.Generator(np.random.PCG64(9)).standard_normal((5, 2))
    got = s2.draw_prior(5, np.random.Generator(np.random.PCG64(9)))
    assert np.array_equal(got[:, 0], np.log(2.0 * np.exp(0.5 * z[:, 0]))) and np.all(got[:, 1] == 0.0)


def test_liu_west_with_shrinkage_one_copies_the_ancestor():
    space, gen, lt, w, anc = _particles(500, 11)
    assert len(np.unique(anc)) < 500
    z = gen.standard_normal(lt.shape)
    out = space.liu_west(lt, w, anc, z, 1.0)
    assert np.array_equal(out, lt[anc])
    assert np.array_equal(space.theta_of(out), space.theta_of(lt)[anc])   # theta' = theta[anc] exactly


def test_liu_west_is_reproducible_fixed_and_bounded():
    space, gen, lt, w, anc = _particles(500, 12)
    z = gen.standard_normal(lt.shape)
    out = space.liu_west(lt, w, anc, z, 0.9)
    space2, gen2, lt2, w2, anc2 = _particles(500, 12)
    assert np.array_equal(out, space2.liu_west(lt2, w2, anc2, gen2.standard_normal(lt2.shape), 0.9))
    assert not np.array_equal(out[:, :2], lt[anc][:, :2])
    assert np.array_equal(out[:, 2], lt[anc][:, 2])                       # the Fixed knob never moves
    th = space.theta_of(out)
    assert np.all(th[:, 2] == np.float64(np.float32(0.75)))
    # bounds hold, also when the kernel would leave them: a wide cloud, a strong kernel
    wide = lt.copy()
    wide[:, 0] = np.linspace(math.log(0.25), math.log(4.0), 500)
    th = space.theta_of(space.liu_west(wide, w, anc, 3.0 * z, 0.6))
    assert np.all((th[:, 0] >= 0.25) & (th[:, 0] <= 4.0)) and np.all((th[:, 1] >= 0.5) & (th[:, 1] <= 1.5))
    assert th[:, 0].min() == 0.25 and th[:, 0].max() == 4.0
    # a knob whose cloud has collapsed (s = 0) does not move
    flat = lt.copy()
    flat[:, 0] = 0.125
    assert np.all(space.liu_west(flat, w, anc, z, 0.9)[:, 0] == 0.125)
    for bad in (0.5, 1.01):
        with pytest.raises(ValueError):
            space.liu_west(lt, w, anc, z, bad)


def test_liu_west_keeps_the_weighted_mean():
    """10^4 synthetic particles: under systematic resampling and the kernel, the mean of log theta' stays at m.  With
    a = (3 delta - 1) / (2 delta): log theta'_k = a x_anc[k] + (1 - a) m + h s z_k, so the mean over k is m + a (mean(x_anc) -
    m) + h s mean(z).  The sigma used: sqrt(a^2 s^2 sum_i w_i^2 + h^2 s^2 / K) -- the kernel's part, h s / sqrt(K), plus a
    bound on the resampling's (systematic resampling's offspring counts vary less than a multinomial's, whose variance of
    mean(x_anc) is s^2 / K <= s^2 sum w_i^2)."""
    K = 10000
    space = ParameterSpace([Knob('beta', 'infectiousness_multiplier', prior=LogNormal(1.0, 0.3), bounds=(1e-3, 1e3))])
    for seed, delta in ((21, 0.98), (22, 0.9), (23, 0.75)):
        gen = np.random.Generator(np.random.PCG64(np.random.SeedSequence([seed, 1])))
        lt = space.draw_prior(K, gen)
        rng = np.random.default_rng(seed)
        w = np.exp(-0.5 * ((lt[:, 0] - 0.2) / 0.25) ** 2) * rng.random(K)
        w /= w.sum()
        anc, _ = filtering.assign_in_place(filtering.systematic_offspring(w, rng.random()))
        out = space.liu_west(lt, w, anc, gen.standard_normal((K, 1)), delta)
        m = float(np.sum(w * lt[:, 0]))
        s = math.sqrt(float(np.sum(w * (lt[:, 0] - m) ** 2)))
        a = (3 * delta - 1) / (2 * delta)
        h = math.sqrt(1 - a * a)
        sigma = math.sqrt(a * a * s * s * float(np.sum(w * w)) + h * h * s * s / K)
        got = float(out[:, 0].mean())
        print('delta %.2f: m %.5f mean(log theta\') %.5f sigma %.5f' % (delta, m, got, sigma))
        assert abs(got - m) < 4.5 * sigma
        # ... and the kernel restores the variance the shrinkage took: var' ~ s^2 (within 10 %: a^2 + h^2 = 1)
        assert abs(float(out[:, 0].var()) / (s * s) - 1.0) < 0.1


def test_filter_with_parameters_on_oracle_b_names_the_header():
    v, ages = filter_util.small_scenario(2000)
    space = ParameterSpace([Knob('beta', 'infectiousness_multiplier', prior=LogNormal(1.0, 0.3))])
    with pytest.raises(eng.EngineError, match=r'reina_params\.h'):
        filtering.particle_filter(v, 3, days=5, window=5, age_counts=ages, engine_factory=PAR, parameters=space)
    r = filtering.particle_filter(v, 3, days=10, window=5, age_counts=ages, engine_factory=PAR, seeds=[5, 6, 7])
    try:
        want = ensemble.run_ensemble(v, [5, 6, 7], 10, age_counts=ages, engine_factory=PAR)
        assert np.array_equal(r.paths(), want)
        assert r.parameters is None and all(w['theta'] is None for w in r.windows)
        with pytest.raises(ValueError, match='learns no parameters'):
            r.parameter_band('beta')
    finally:
        r.close()


def test_parameter_ensemble_on_oracle_b_equals_single_contexts():
    v, ages = filter_util.small_scenario(20000)
    space = ParameterSpace([Knob('beta', 'infectiousness_multiplier'), Knob('old', 'p_severe_given_symptomatic', ages=(60, 100))])
    thetas = np.array([[1.0, 1.0], [1.6, 0.5], [0.6, 3.0]], dtype=np.float32)
    seeds = [31, 32, 33]
    hist, ctxs = ensemble.run_parameter_ensemble(v, thetas, seeds, 40, space, age_counts=ages, engine_factory=PAR)
    assert hist.shape == (3, 40, eng.COUNTER_WORDS)
    base = simulation.make_context(v, age_counts=ages, seed=1, ipc=None, engine_factory=PAR)._disease
    for m, (sd, th) in enumerate(zip(seeds, thetas)):
        block, _ = par.expand_numpy(base, space, th, A, V)
        assert par.disease_bytes(ctxs[m]._disease) == par.disease_bytes(block)
        one = simulation.make_context(v, age_counts=ages, seed=sd, ipc='auto', engine_factory=PAR, disease=block)
        assert np.array_equal(one.run(40), hist[m]), m
    # member 0 ran under the base itself
    plain = simulation.make_context(v, age_counts=ages, seed=31, ipc='auto', engine_factory=PAR)
    assert np.array_equal(plain.run(40), hist[0])
    inf = filter_util.totals(hist, 'all_infected')[:, -1]
    assert len(set(inf.tolist())) >= 2, inf
