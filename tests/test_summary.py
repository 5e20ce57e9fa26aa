"""Ensemble summaries on the CPU: the numpy specification (reina_model_amd/summary.py: summarise_numpy) against plain Python
loops over the definition, the rank rule against numpy's inverted CDF, the header against the module, the refusals of the
Python layer, and run_group_plan(summary=...) on oracle B against the history the same run returns without it.  Every
comparison is of integers and exact."""
import os
import re

import numpy as np
import pytest

import par_backend
import summary_util as su
from filter_util import small_scenario
from reina_model_amd import engine as eng
from reina_model_amd import ensemble, simulation, summary as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- 1. the specification

@pytest.mark.parametrize('pattern', su.PATTERNS)
@pytest.mark.parametrize('K,days,nr_ages,G,Q,T', [(1, 1, 1, 1, 1, 0), (3, 4, 5, 2, 16, 6), (5, 2, 7, 4, 1, 3)])
def test_spec_equals_walker(pattern, K, days, nr_ages, G, Q, T):
    h = su.history(K, days, nr_ages, pattern)
    spec = su.spec_for(h, nr_ages, G, Q, T)
    lay = sm.Layout(spec, K, days, nr_ages)
    assert (lay.G, lay.Q, lay.T, lay.S) == (G, Q, T, eng.C_NR * (1 + G) + eng.S_NR)
    w = sm.summarise_numpy(h, nr_ages, spec)
    su.assert_words(w, su.walk(h, nr_ages, lay), lay)
    # a list of members' arrays is the same history
    su.assert_words(sm.summarise_numpy([h[m] for m in range(K)], nr_ages, spec), w, lay)


def test_wrapping_sums_and_extremes_are_what_the_patterns_say():
    h = su.history(4, 3, 101, 'wrap')
    lay = sm.Layout(sm.SummarySpec(), 4, 3, 101)
    ser = sm.series_numpy(h, 101, lay.table, lay.G)
    true = h[:, :, :101].astype(np.int64).sum(axis=-1)
    assert (true > 2 ** 31).all() and np.array_equal(ser[:, :, 0], ((true + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int32))
    e = sm.summarise(su.history(6, 4, 128, 'extremes'), 128, sm.SummarySpec())
    assert e.peak[:, e.layout.S - eng.S_NR:, 0].max() == su.I32_MAX and e.order[:, e.layout.S - eng.S_NR:, 0].min() == su.I32_MIN


@pytest.mark.parametrize('K', (1, 2, 3, 7, 64, 100, 129, 1024))
def test_rank_rule_is_the_inverted_cdf(K):
    x = np.random.default_rng(K).permutation(K) * 3 - K      # distinct values: a value names its rank
    for q in (0.0, 0.01, 0.05, 0.25, 1 / 3, 0.5, 0.75, 0.9, 0.95, 0.99, 1.0):
        r = sm.rank(q, K)
        assert 0 <= r <= K - 1
        assert np.sort(x)[r] == np.quantile(x, q, method='inverted_cdf'), (q, K)
    with pytest.raises(ValueError):
        sm.rank(1.5, K)


# ---------------------------------------------------------------------------------------------- 2. the header, the library

def _header():
    with open(os.path.join(ROOT, 'include', 'reina_summary.h')) as fh:
        return fh.read()


def test_header_constants_and_offsets_equal_the_module():
    h = _header()
    defs = dict(re.findall(r'#define (REINA_SUMMARY_\w+) (\d+)\b', h))
    for c, v in (('VERSION', sm.SUMMARY_VERSION), ('MAX_MEMBERS', sm.MAX_MEMBERS), ('MAX_GROUPS', sm.MAX_GROUPS),
                 ('MAX_RANKS', sm.MAX_RANKS), ('MAX_THRESHOLDS', sm.MAX_THRESHOLDS), ('PEAK_FIELDS', sm.PEAK_FIELDS)):
        assert int(defs['REINA_SUMMARY_' + c]) == v, c
    env = {k: int(v) for k, v in defs.items()}
    env.update(REINA_C_NR=eng.C_NR, REINA_S_NR=eng.S_NR)
    clean = lambda e: re.sub(r'\b(\d+)u\b', r'\1', e.replace('(size_t)', ''))
    series = clean(re.search(r'#define REINA_SUMMARY_SERIES\(G\) (.+)$', h, re.M).group(1))
    macros = dict(re.findall(r'#define (REINA_SUMMARY_\w+)\(K, days, S, Q, T\) (.+)$', h, re.M))
    names = ('ORDER', 'SUM', 'PEAK', 'FINAL', 'EXCEED', 'FIRST_EXCEED', 'REPORT_WORDS')
    assert sorted(macros) == sorted('REINA_SUMMARY_' + n for n in names)
    head = clean(re.search(r'#define REINA_SUMMARY_HEAD_BYTES\(K\) (.+)$', h, re.M).group(1))
    scratch = clean(re.search(r'#define REINA_SUMMARY_SCRATCH_BYTES\(K, days, S\) (.+)$', h, re.M).group(1))
    fns = (sm.order_offset, sm.sum_offset, sm.peak_offset, sm.final_offset, sm.exceed_offset, sm.first_exceed_offset, sm.report_words)
    for K, days, G, Q, T in ((1, 1, 1, 0, 0), (3, 5, 2, 2, 4), (128, 365, 9, 5, 3), (1024, eng.MAX_DAYS, 16, 16, 32)):
        S = eval(series, dict(G=G), env)
        assert S == sm.n_series(G)
        args = dict(K=K, days=days, S=S, Q=Q, T=T)
        val = {}
        for n, f in zip(names, fns):
            e = re.sub(r'(REINA_SUMMARY_\w+)\(K, days, S, Q, T\)', lambda m: str(val[m.group(1)]), clean(macros['REINA_SUMMARY_' + n]))
            val['REINA_SUMMARY_' + n] = eval(e, dict(args), env)
            assert val['REINA_SUMMARY_' + n] == f(K, days, S, Q, T), n
        hb = eval(head, dict(K=K), env)
        assert hb == sm.head_bytes(K) and hb % 256 == 0 and hb >= 512 + 8 * K
        sb = eval(scratch.replace('REINA_SUMMARY_HEAD_BYTES(K)', str(hb)), dict(args), env)
        assert sb == sm.scratch_bytes(K, days, S) and sb >= hb + 4 * days * K * S
        lay = sm.Layout(sm.SummarySpec((0.5,) * Q, su.groups(G, 101), [('dead', 1)] * T), K, days, 101)
        assert lay.words == val['REINA_SUMMARY_REPORT_WORDS'] and lay.S == S
    # what the issue sizes the result at: a year of 128 members, 9 groups, 5 quantiles is a few MB at the most
    assert sm.report_words(128, 365, sm.n_series(9), 5, 3) * 8 < 6_000_000


def _declared_functions():
    text = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    return sorted(set(re.findall(r'\b(reina_[a-z_]+)\s*\(', text)))


def test_library_exports_every_function_the_header_declares():
    from reina_model_amd import build
    assert _declared_functions() == sorted('reina_' + f for f in sm.SUMMARY_FUNCTIONS)
    build.build()
    lib = eng.load_hip_library()
    for fn in _declared_functions():
        assert hasattr(lib, fn), fn
    f = sm.bind_summary_abi(lib, 'reina_')
    assert f is not None and f['summary_version']() == sm.SUMMARY_VERSION == 1
    assert eng.bind_abi(lib, 'reina_')['abi_version']() == 7
    assert sm.bind_summary_abi(par_backend.lib(), 'par_') is None
    assert os.path.join(ROOT, 'include', 'reina_summary.h') in build.DEPS


# ---------------------------------------------------------------------------------------------- 3. refusals (host side)

def test_refusals_of_the_python_layer():
    h = su.history(3, 2, 10, 'random')
    ok = sm.SummarySpec()
    with pytest.raises(ValueError, match='at most 16 quantiles'):
        sm.SummarySpec(quantiles=[0.5] * 17)
    with pytest.raises(ValueError, match='quantile level'):
        sm.SummarySpec(quantiles=[-0.1])
    with pytest.raises(ValueError, match='at most 32 thresholds'):
        sm.SummarySpec(thresholds=[('dead', 1)] * 33)
    with pytest.raises(ValueError, match='unknown attribute'):
        sm.SummarySpec(thresholds=[('nothing', 1)])
    with pytest.raises(ValueError, match='int32'):
        sm.SummarySpec(thresholds=[('dead', 2 ** 31)])
    with pytest.raises(ValueError, match='a threshold is'):
        sm.SummarySpec(thresholds=[('dead',)])
    with pytest.raises(ValueError, match='unknown age group'):
        sm.summarise_numpy(h, 10, sm.SummarySpec(thresholds=[('dead', 'nobody', 1)]))
    with pytest.raises(ValueError, match='no age groups'):
        sm.summarise_numpy(h, 10, sm.SummarySpec(thresholds=[('beds', '0-9', 1)]))
    with pytest.raises(ValueError, match='age groups are'):
        sm.summarise_numpy(h, 10, sm.SummarySpec(age_groups=np.arange(10) + 8))
    with pytest.raises(ValueError, match='ages given'):
        sm.summarise_numpy(h, 10, sm.SummarySpec(age_groups=[0, 1]))
    with pytest.raises(ValueError, match='nr_ages'):
        sm.summarise_numpy(h, 129, ok)
    with pytest.raises(ValueError, match='members'):
        sm.summarise_numpy(np.zeros((1025, 1, eng.COUNTER_WORDS), dtype=np.int32), 10, ok)
    with pytest.raises(ValueError, match='days'):
        sm.summarise_numpy(np.zeros((2, 0, eng.COUNTER_WORDS), dtype=np.int32), 10, ok)
    with pytest.raises(ValueError, match='a history is'):
        sm.summarise_numpy(np.zeros((2, 3, 7), dtype=np.int32), 10, ok)
    s = sm.summarise(h, 10, sm.SummarySpec(thresholds=[('dead', 5)]))
    with pytest.raises(ValueError, match='not asked for'):
        s.exceedance('dead', 6)
    with pytest.raises(ValueError, match='has .* words'):
        sm.EnsembleSummary(s.words[:-1], s.layout)


# ---------------------------------------------------------------------------------------------- 4. runs on oracle B

def _oracle(v, ages, seed):
    return simulation.make_context(v, age_counts=ages, seed=seed, engine_factory=par_backend.par_engine_factory, ipc='auto')


def _spec(ctx):
    return sm.SummarySpec(thresholds=[('in_icu', 1), ('infected', ctx.age_group_labels[3], 2), ('available_icu', 0), ('dead', 10 ** 6)])


def test_group_run_with_a_summary_equals_the_summary_of_its_history():
    v, ages = small_scenario(3000)
    seeds, days = range(8), 30
    a = [_oracle(v, ages, s) for s in seeds]
    hist = ensemble.run_group_plan(a, _oracle(v, ages, 0).make_plan(days))
    b = [_oracle(v, ages, s) for s in seeds]
    spec = _spec(b[0])
    got = ensemble.run_group_plan(b, _oracle(v, ages, 0).make_plan(days), summary=spec)
    assert isinstance(got, sm.EnsembleSummary) and (got.n_members, got.days) == (8, days)
    su.assert_words(got.words, sm.summarise_numpy(hist, b[0].nr_ages, spec, ctx=b[0]), got.layout)
    for x, y in zip(a, b):   # the summary changes nothing in the run
        assert np.array_equal(x.engine.read_counters(), y.engine.read_counters()) and x.day == y.day == days
    # the accessors read the block: the band against numpy on the history, peaks, finals, exceedance
    tot = hist[:, :, eng.C_NAMES.index('infected') * eng.MAX_AGES:][:, :, :eng.MAX_AGES].astype(np.int64).sum(axis=2)
    band = got.band('infected')
    assert list(band.columns) == list(spec.quantiles) and str(band.index[0]) == v['start_date']
    for q in spec.quantiles:
        assert np.array_equal(band[q].to_numpy(), np.quantile(tot, q, axis=0, method='inverted_cdf'))
    assert np.allclose(got.mean('infected').to_numpy(), tot.mean(axis=0))
    pk = got.peaks('infected')
    assert np.array_equal(pk['value'].to_numpy(), tot.max(axis=1)) and pk['date'].iloc[0] == got.dates()[int(tot[0].argmax())]
    assert np.array_equal(got.final('infected').to_numpy(), tot[:, -1])
    icu = hist[:, :, eng.C_NAMES.index('in_icu') * eng.MAX_AGES:][:, :, :eng.MAX_AGES].astype(np.int64).sum(axis=2)
    assert np.allclose(got.exceedance('in_icu', 1).to_numpy(), (icu > 1).mean(axis=0))
    assert got.ever_exceeds('in_icu', 1) == (icu > 1).any(axis=1).mean() and got.ever_exceeds('dead', 10 ** 6) == 0.0
    first = got.first_exceed_dates('in_icu', 1)
    assert [d is None for d in first] == list(~(icu > 1).any(axis=1))
    assert got.frame().shape == (days, eng.C_NR * len(spec.quantiles))
    with pytest.raises(ValueError, match='record_history'):
        ensemble.run_group_plan(b, _oracle(v, ages, 0).make_plan(2), record_history=False, summary=spec)
    with pytest.raises(ValueError, match='SummarySpec'):
        ensemble.run_group_plan(b, _oracle(v, ages, 0).make_plan(2), summary=(0.5,))


def test_ensemble_routes_with_a_summary_equal_the_summary_of_their_history():
    v, ages = small_scenario(3000)
    seeds, days = [3, 1, 4, 15, 9], 12
    kw = dict(age_counts=ages, engine_factory=par_backend.par_engine_factory)
    ref = _oracle(v, ages, 0)
    spec = _spec(ref)
    hist = ensemble.run_ensemble(v, seeds, days, concurrent=2, **kw)
    got = ensemble.run_ensemble(v, seeds, days, concurrent=2, summary=spec, **kw)      # chunks of 2, 2, 1
    su.assert_words(got.words, sm.summarise_numpy(hist, ref.nr_ages, spec, ctx=ref), got.layout)
    assert got.members == seeds and list(got.peaks('dead').index) == seeds
    # branches of a snapshot
    past = _oracle(v, ages, 2)
    past.run(10)
    snap = past.snapshot()
    hist, _ = ensemble.run_branches(snap, v, seeds, days, **kw)
    got, ctxs = ensemble.run_branches(snap, v, seeds, days, summary=spec, **kw)
    su.assert_words(got.words, sm.summarise_numpy(hist, ref.nr_ages, spec, ctx=ref), got.layout)
    assert got.start_day == 10 and len(ctxs) == len(seeds)
