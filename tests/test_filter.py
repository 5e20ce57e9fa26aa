"""The particle filter (reina_model_amd/filtering.py) on the CPU: observations and their alignment, the negative-binomial
term, systematic resampling and its in-place assignment, the numpy clone (the specification of reina_group_clone) on
synthetic states and as a continuation of a run on oracle B, the filter without observations, and its refusals."""
import json
import os
from datetime import date, timedelta

import numpy as np
import pandas as pd
import pytest

import filter_util
import par_backend
import snap_util
from reina_model_amd import datasets, engine as eng, ensemble, filtering, simulation

PAR = par_backend.par_engine_factory
DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'reina_model_amd', 'data')


@pytest.mark.parametrize('area,fname', [('HUS', 'fi_hus.json'), ('Turku', 'fi_turku.json'),
                                        ('Varsinais-Suomi', 'fi_varsinais-suomi.json')])
def test_detected_cases_are_the_bundled_rows(area, fname):
    with open(os.path.join(DATA, fname)) as f:
        d = json.load(f)
    df = datasets.get_detected_cases(area)
    assert list(df.columns) == ['dead', 'in_icu', 'in_ward', 'all_detected']
    assert len(df) == len(d['case_rows'])
    for (t, dead, icu, ward, conf), (idx, row) in zip(d['case_rows'], df.iterrows()):
        assert idx == date.fromisoformat(t)
        assert list(row) == [dead, icu, ward, conf]
    assert datasets.get_detected_cases({'area_name': area}).equals(df)


def test_alignment_with_gaps():
    start = '2020-02-18'
    d0 = date.fromisoformat(start)
    idx = [d0 - timedelta(days=3), d0, d0 + timedelta(days=2), d0 + timedelta(days=9), d0 + timedelta(days=5),
           d0 + timedelta(days=40)]
    df = pd.DataFrame({'all_detected': [1, 2, 5, 9, np.nan, 50], 'in_ward': [0, 1, 1, 2, 3, 4]}, index=idx)
    al = filtering.align(df, start, 0, 30, ('all_detected', 'in_ward'))
    assert al['all_detected'][0].tolist() == [0, 2, 9]          # before day 0, missing and beyond the horizon dropped
    assert al['all_detected'][1].tolist() == [2, 5, 9]
    assert al['in_ward'][0].tolist() == [0, 2, 5, 9]            # sorted by date
    assert al['in_ward'][1].tolist() == [1, 1, 3, 2]
    al = filtering.align(df, start, 3, 30, ('in_ward',))         # a horizon starting later (a snapshot's day)
    assert al['in_ward'][0].tolist() == [5, 9]
    # string dates work as well
    df2 = pd.DataFrame({'in_ward': [7]}, index=['2020-02-20'])
    assert filtering.align(df2, start, 0, 10, ('in_ward',))['in_ward'][0].tolist() == [2]


def test_scoring_of_increments_and_levels():
    """cumulative streams: increments between consecutive observed rows, across windows through the carried value; levels:
    the level.  A term belongs to the window of its later row."""
    K = 3
    rng = np.random.default_rng(5)
    hist = np.zeros((K, 20, eng.COUNTER_WORDS), dtype=np.int32)
    ad = eng.C_NAMES.index('all_detected') * eng.MAX_AGES
    iw = eng.C_NAMES.index('in_ward') * eng.MAX_AGES
    cum = np.cumsum(rng.integers(0, 20, size=(K, 20)), axis=1)
    hist[:, :, ad + 3] = cum // 2
    hist[:, :, ad + 40] = cum - cum // 2
    ward = rng.integers(0, 9, size=(K, 20))
    hist[:, :, iw + 7] = ward
    rows = [1, 4, 8, 15]
    obs_ad = [3, 10, 30, 31]
    obs_iw = [2, 0, 5, 1]
    al = {'all_detected': (np.array(rows), np.array(obs_ad, float)), 'in_ward': (np.array(rows), np.array(obs_iw, float))}
    model = filtering.ObservationModel({'all_detected': 4.0, 'in_ward': 2.5}, floor=0.5)
    sc = filtering._Scorer(model, al, K)
    got = sc.score(hist[:, 0:7], 0) + sc.score(hist[:, 7:14], 7) + sc.score(hist[:, 14:20], 14)
    want = np.zeros(K)
    for j, r in enumerate(rows):
        want += filtering.nb_logpmf(obs_iw[j], np.maximum(ward[:, r], 0.5), 2.5)
        if j:
            mu = np.maximum(cum[:, r] - cum[:, rows[j - 1]], 0.5)
            want += filtering.nb_logpmf(obs_ad[j] - obs_ad[j - 1], mu, 4.0)
    np.testing.assert_allclose(got, want, rtol=1e-13)


def test_nb_term_equals_scipy():
    stats = pytest.importorskip('scipy.stats')
    rng = np.random.default_rng(1)
    y = rng.integers(0, 2000, size=2000)                 # (daily to weekly counts of a hospital district)
    mu = np.exp(rng.uniform(-1, 7.5, size=2000))
    r = np.exp(rng.uniform(-1, 4, size=2000))
    got = np.array([filtering.nb_logpmf(y[k], mu[k], r[k]) for k in range(len(y))])
    want = stats.nbinom.logpmf(y, r, r / (r + mu))
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
    model = filtering.ObservationModel({'in_icu': 3.0}, floor=0.5)
    assert model.logpmf(2, 0, 'in_icu') == filtering.nb_logpmf(2, 0.5, 3.0)


@pytest.mark.parametrize('K', (2, 3, 8, 64, 1000))
def test_systematic_resampling(K):
    rng = np.random.default_rng(K)
    for trial in range(50):
        w = rng.exponential(size=K) ** (1 + trial % 4 * 2)
        w[rng.random(K) < 0.2] = 0
        if w.sum() == 0:
            w[0] = 1
        w = w / w.sum()
        u = rng.random()
        c = filtering.systematic_offspring(w, u)
        assert c.sum() == K
        assert np.all(c >= np.floor(K * w - 1e-9)) and np.all(c <= np.ceil(K * w + 1e-9))
        anc, pairs = filtering.assign_in_place(c)
        assert np.array_equal(np.bincount(anc, minlength=K), c)
        alive = np.flatnonzero(c > 0)
        assert np.array_equal(anc[alive], alive)                          # every survivor keeps itself
        dst = [d for d, _ in pairs]
        src = [s for _, s in pairs]
        assert sorted(dst) == dst and set(dst) == set(np.flatnonzero(c == 0))   # only the dead are written
        assert not set(dst) & set(src)                                    # no source is a destination
        assert src == sorted(src)                                         # surplus in ascending order
        for d, s in pairs:
            assert anc[d] == s


def _pf(v, ages, K, obs=None, **kw):
    return filtering.particle_filter(v, K, observations=obs, engine_factory=PAR, age_counts=ages, **kw)


def test_filter_is_reproducible_from_filter_seed():
    v, ages = filter_util.small_scenario()
    truth = simulation.make_context(v, age_counts=ages, seed=901, ipc='auto', engine_factory=PAR)
    obs = filter_util.observations(truth.run(40), v['start_date'], range(8, 40))
    model = filtering.ObservationModel({'all_detected': 5.0, 'in_ward': 5.0})
    r1 = _pf(v, ages, 4, obs, obs_model=model, days=40, filter_seed=3, seeds=[11, 12, 13, 14])
    r2 = _pf(v, ages, 4, obs, obs_model=model, days=40, filter_seed=3, seeds=[11, 12, 13, 14])
    assert any(w['resampled'] for w in r1.windows)
    assert np.array_equal(r1.ancestors, r2.ancestors)
    assert np.array_equal(r1.loglik, r2.loglik) and r1.log_evidence == r2.log_evidence
    assert np.array_equal(r1.paths(), r2.paths())
    assert r1.paths().shape == (4, 40, eng.COUNTER_WORDS)
    # the paths are the members' own rows, traced through the ancestors
    last = r1.windows[-1]
    assert np.array_equal(r1.paths()[:, -last['days']:], last['history'][last['ancestors']])
    q = r1.quantiles('all_detected', (0.05, 0.5, 0.95))
    assert list(q.columns) == [0.05, 0.5, 0.95] and len(q) == 40
    assert np.all(q[0.05].to_numpy() <= q[0.95].to_numpy())
    fc = r1.forecast(10)
    assert fc.shape == (4, 10, eng.COUNTER_WORDS) and r1.paths().shape == (4, 50, eng.COUNTER_WORDS)
    r1.close()
    r2.close()


def _engine_pair(n, pattern_dst, pattern_src, seed):
    a = snap_util.make_context(n, engine_factory=PAR)
    b = snap_util.make_context(n, engine_factory=PAR)
    mq = a.engine.config.max_queue
    sa = snap_util.synthetic_state(n, mq, pattern_dst, seed=seed, queues=True)
    sb = snap_util.synthetic_state(n, mq, pattern_src, seed=seed + 1, queues=True)
    snap_util.write_state(a.engine, sa)
    snap_util.write_state(b.engine, sb)
    rng = np.random.default_rng(seed)
    for e in (a.engine, b.engine):
        for name in ('active_bits', 'infected_bits'):
            e.tensors[name].view(np.uint32)[:] = rng.integers(0, 1 << 32, size=len(e.tensors[name]), dtype=np.uint64)
    return a, b


def expected_clone(dst, src, n, max_queue):
    """the clone written agent by agent from the header's table (include/reina_filter.h)"""
    out = {k: v.copy() for k, v in dst.items()}
    for i in range(n):
        if src['hot'][i]:
            out['cold'][i] = src['cold'][i]
            out['infectees'][i] = src['infectees'][i]
        elif dst['hot'][i]:
            out['cold'][i] = snap_util.COLD_DEFAULT
            out['infectees'][i] = snap_util.NONE
        out['hot'][i] = src['hot'][i]
    out['counters'] = src['counters'].copy()
    out['control'] = src['control'].copy()
    for k, q in enumerate(('queue0', 'queue1', 'level1')):
        ln = min(max(int(np.int32(src['control'][2 + k])), 0), max_queue)
        out[q][:ln] = src[q][:ln]
    T16 = 16 * snap_util.n_tiles(n)
    for name in ('active_bits', 'infected_bits'):
        out[name][:T16] = src[name][:T16]
    return out


@pytest.mark.parametrize('n', (1, 511, 512, 513, 2 * 512 + 7))
@pytest.mark.parametrize('pats', [('random', 'random'), ('full', 'empty'), ('empty', 'full'), ('edges', 'alternating')])
def test_numpy_clone_on_synthetic_states(n, pats):
    a, b = _engine_pair(n, pats[0], pats[1], seed=n)
    dst, src = filter_util.carried(a.engine), filter_util.carried(b.engine)
    mq = a.engine.config.max_queue
    want = expected_clone(dst, src, n, mq)
    group = eng.EngineGroup([a.engine, b.engine])
    filtering.clone_group(group, [(0, 1)])
    group.close()
    got = filter_util.carried(a.engine)
    for name, w in want.items():
        assert np.array_equal(got[name], w), name
    after = filter_util.carried(b.engine)
    for name in src:
        assert np.array_equal(after[name], src[name]), name   # the source is read only


def test_numpy_clone_continues_like_a_restored_snapshot():
    """clone a -> m, run D days as a group: member m = a restore of a snapshot of a into a fresh Context with m's seed"""
    v, ages = filter_util.small_scenario()
    hist, member, want, ref = filter_util.continuation(v, ages, [31, 32, 33], a=0, m=2, cut=25, days=20, engine_factory=PAR)
    assert np.array_equal(hist, want)
    filter_util.assert_same_day_state(member, ref, planes=False)


def test_no_observations_is_run_group_plan():
    v, ages = filter_util.small_scenario()
    seeds = [5, 6, 7]
    r = _pf(v, ages, 3, None, days=30, seeds=seeds, window=7)
    assert all(not w['resampled'] for w in r.windows) and r.log_evidence == 0.0
    assert [w['days'] for w in r.windows] == [7, 7, 7, 7, 2]
    setup = ensemble.Setup(ages, engine_factory=PAR, ipc='auto')
    ctxs = setup.members(v, seeds)
    want = ensemble.run_group_plan(ctxs, setup.planner(v, seeds[0]).make_plan(30))
    assert np.array_equal(r.paths(), want)
    for c, w in zip(r.contexts, ctxs):
        assert np.array_equal(c.engine.read_counters(), w.engine.read_counters())
    r.close()


def test_refusals():
    v, ages = filter_util.small_scenario(3000)
    d0 = date.fromisoformat(v['start_date'])
    obs = pd.DataFrame({'all_detected': [1, 4]}, index=[d0 + timedelta(days=3), d0 + timedelta(days=9)])
    with pytest.raises(ValueError, match='2 particles'):
        _pf(v, ages, 1, obs, days=10)
    with pytest.raises(ValueError, match='unknown stream'):
        _pf(v, ages, 2, obs, obs_model=filtering.ObservationModel({'hospitalized': 3.0}), days=10)
    with pytest.raises(ValueError, match='unknown stream'):
        _pf(v, ages, 2, obs, obs_model={'confirmed': 3.0}, days=10)
    with pytest.raises(ValueError, match='no column'):
        _pf(v, ages, 2, obs, obs_model=filtering.ObservationModel({'dead': 3.0}), days=10)
    late = pd.DataFrame({'all_detected': [1]}, index=[d0 + timedelta(days=50)])
    early = pd.DataFrame({'all_detected': [1]}, index=[d0 - timedelta(days=5)])
    for o in (late, early):
        with pytest.raises(ValueError, match='no observed date inside the horizon'):
            _pf(v, ages, 2, o, days=10)
    from reina_model_amd import sharding
    with pytest.raises(ValueError, match='sharded'):
        _pf(v, ages, 2, obs, days=10, comm=sharding.InProcessComm(0, 2, [None, None], attribution='mirror'))
    # clone pair lists
    ctxs = [snap_util.make_context(700, engine_factory=PAR) for _ in range(4)]
    group = eng.EngineGroup([c.engine for c in ctxs])
    for pairs, why in (([(4, 0)], 'out of range'), ([(1, 0), (1, 2)], 'twice'), ([(1, 0), (0, 2)], 'also a destination'),
                       ([(2, 2)], 'also a destination'), ([(-1, 0)], 'out of range')):
        with pytest.raises(ValueError, match=why):
            filtering.clone_group(group, pairs)
    group.close()

