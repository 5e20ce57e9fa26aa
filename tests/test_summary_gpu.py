"""Ensemble summaries on the GPU: the library's kernels (reina_summary: k_summary_series, k_summary_peak, k_summary_order)
against the numpy specification word for word on synthetic histories -- no engine involved, so the shapes are the smallest at
which the kernels can go wrong --, the refusals of the C ABI, and real ensembles whose summary must equal the summary of the
history an identical run returns, and must change nothing in the run."""
import ctypes

import numpy as np
import pytest

import summary_util as su
from filter_util import small_scenario
from reina_model_amd import engine as eng
from reina_model_amd import ensemble, simulation, summary as sm

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 200, 1024)


def _cases():
    """a covering set, not the product: every K four times, and against it days, nr_ages, G, Q, T, the value pattern and the
    members' placement cycling with periods that share no factor with 11"""
    out = []
    for i in range(4 * len(KS)):
        K = KS[i % len(KS)]
        days = (1, 2, 7)[i % 3] if K < 1024 else (1, 2)[i % 2]
        out.append((K, days, (1, 101, 128)[(i // 2) % 3], (1, 4, 16)[(i // 3) % 3], (1, 16)[i % 2], (0, 32)[(i // 2) % 2],
                    su.PATTERNS[(i + i // 6) % len(su.PATTERNS)], ('contiguous', 'separate')[(i // 4) % 2]))
    return out


def _id(c):
    return 'K%d-d%d-a%d-G%d-Q%d-T%d-%s-%s' % c


@pytest.mark.parametrize('case', _cases(), ids=_id)
def test_kernels_equal_spec_on_synthetic_histories(case):
    import torch
    K, days, nr_ages, G, Q, T, pattern, placement = case
    h = su.history(K, days, nr_ages, pattern, seed=K + days)
    spec = su.spec_for(h, nr_ages, G, Q, T, seed=K)
    assert sm.library() is not None
    if placement == 'contiguous':
        order = np.arange(K)
        dev = torch.from_numpy(h).to('cuda:0')
        parts, given = [dev], dev
    else:   # one allocation a member, handed over in another order
        order = np.random.default_rng(K).permutation(K)
        parts = [torch.from_numpy(h[m].copy()).to('cuda:0') for m in order]
        given = parts
    got = sm.summarise(given, nr_ages, spec)
    lay = got.layout
    assert (lay.K, lay.days, lay.G, lay.Q, lay.T) == (K, days, G, Q, T)
    su.assert_words(got.words, sm.summarise_numpy(h[order], nr_ages, spec), lay)
    for p, m in zip(parts, [None] if placement == 'contiguous' else order):   # the rows are read, never written
        assert np.array_equal(p.cpu().numpy(), h if m is None else h[m])
    if Q == 16:
        assert lay.ranks[0] == K - 1 and lay.ranks[1] == 0 and lay.ranks[2] == lay.ranks[3]


# ---------------------------------------------------------------------------------------------- refusals of the C ABI

def test_refusals_through_the_c_abi():
    import torch
    f = sm.library()
    K, days, nr_ages, G = 3, 2, 10, 2
    S = sm.n_series(G)
    h = torch.from_numpy(su.history(K, days, nr_ages, 'random')).to('cuda:0')
    row = 4 * eng.COUNTER_WORDS
    scratch = torch.empty(sm.scratch_bytes(K, days, S) + 16, dtype=torch.uint8, device='cuda:0')
    rep = torch.full((sm.report_words(K, days, S, 2, 1) + 2,), -77, dtype=torch.int64, device='cuda:0')
    stream = torch.cuda.current_stream().cuda_stream
    good = dict(bases=[h.data_ptr() + m * days * row for m in range(K)], K=K, days=days, nr_ages=nr_ages,
                table=np.arange(eng.MAX_AGES, dtype=np.uint8) % G, G=G, ranks=np.array([0, 2], dtype=np.uint32), Q=2,
                thr=[(5, 1)], T=1, scratch=scratch.data_ptr(), rep=rep.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        bases = (ctypes.c_void_p * max(len(a['bases']), 1))(*a['bases']) if a['bases'] is not None else None
        thr = (sm.Threshold * max(len(a['thr']), 1))(*[sm.Threshold(s, v) for s, v in a['thr']]) if a['thr'] is not None else None
        table = np.ascontiguousarray(a['table'], dtype=np.uint8) if a['table'] is not None else None
        ranks = np.ascontiguousarray(a['ranks'], dtype=np.uint32) if a['ranks'] is not None else None
        rc = f['summary'](bases, a['K'], a['days'], a['nr_ages'], table.ctypes.data if table is not None else None, a['G'],
                          ranks.ctypes.data if ranks is not None else None, a['Q'], thr, a['T'], a['scratch'], a['rep'], stream)
        return rc, (f['last_error']() or b'').decode()

    bad_table = good['table'].copy()
    bad_table[nr_ages - 1] = G
    refused = [
        (dict(K=0), 'K must be'), (dict(K=1025, bases=good['bases'] * 342), 'K must be'),
        (dict(days=0), 'days must be'), (dict(days=eng.MAX_DAYS + 1), 'days must be'),
        (dict(nr_ages=0), 'nr_ages must be'), (dict(nr_ages=eng.MAX_AGES + 1), 'nr_ages must be'),
        (dict(G=0), 'n_groups must be'), (dict(G=17), 'n_groups must be'),
        (dict(Q=17), 'n_ranks'), (dict(T=33), 'n_thresholds'),
        (dict(table=bad_table), "an age's group"),
        (dict(ranks=np.array([0, K], dtype=np.uint32)), 'a rank'),
        (dict(thr=[(S, 0)]), "a threshold's series"),
        (dict(bases=None), 'null'), (dict(table=None), 'null'), (dict(ranks=None), 'null'), (dict(thr=None), 'null'),
        (dict(scratch=None), 'null'), (dict(rep=None), 'null'),
        (dict(bases=[good['bases'][0], 0, good['bases'][2]]), 'null'),
        (dict(bases=[good['bases'][0], good['bases'][1] + 4, good['bases'][2]]), '16-byte aligned'),
        (dict(scratch=good['scratch'] + 8), '16-byte aligned'), (dict(rep=good['rep'] + 8), '16-byte aligned'),
    ]
    for kw, text in refused:
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith('reina_summary: ') and text in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert bool((rep == -77).all()), 'a refused call queued something'
    # and the same arguments unharmed are taken: every word of the block is written
    rc, msg = call()
    assert rc == 0, msg
    torch.cuda.synchronize()
    w = rep.cpu().numpy()
    assert (w[-2:] == -77).all()
    spec = sm.SummarySpec((0.0, 1.0), good['table'][:nr_ages], ())
    lay = sm.Layout(spec, K, days, nr_ages)
    lay.thresholds, lay.T = [(5, 1)], 1
    lay.offsets = [g(K, days, S, 2, 1) for g in (sm.order_offset, sm.sum_offset, sm.peak_offset, sm.final_offset, sm.exceed_offset,
                                                 sm.first_exceed_offset, sm.report_words)]
    lay.words = lay.offsets[-1]
    su.assert_words(w[:-2], sm._words_numpy(h.cpu().numpy(), lay), lay)


# ---------------------------------------------------------------------------------------------- real runs

def _mk(v, ages, seed):
    return simulation.make_context(v, age_counts=ages, seed=seed, ipc='auto')


def _spec(ctx):
    return sm.SummarySpec(thresholds=[('in_icu', 1), ('infected', ctx.age_group_labels[3], 2), ('available_icu', 0), ('dead', 10 ** 6)])


def _finals(ctxs):
    return np.stack([c.engine.read_counters() for c in ctxs])


def test_group_run_with_a_summary_equals_the_summary_of_its_history():
    v, ages = small_scenario()
    seeds, days = range(16), 40
    a = [_mk(v, ages, s) for s in seeds]
    hist = ensemble.run_group_plan(a, _mk(v, ages, 0).make_plan(days))
    b = [_mk(v, ages, s) for s in seeds]
    spec = _spec(b[0])
    assert b[0].engine.summary_f is not None
    got = ensemble.run_group_plan(b, _mk(v, ages, 0).make_plan(days), summary=spec)
    assert isinstance(got, sm.EnsembleSummary) and (got.n_members, got.days) == (16, days)
    su.assert_words(got.words, sm.summarise_numpy(hist, b[0].nr_ages, spec, ctx=b[0]), got.layout)
    assert np.array_equal(_finals(a), _finals(b)), 'the summary changed the run'
    assert got.ever_exceeds('dead', 10 ** 6) == 0.0 and str(got.band('infected').index[0]) == v['start_date']


def test_chunked_ensemble_with_a_summary_equals_the_summary_of_its_history():
    v, ages = small_scenario()
    seeds, days = list(range(20, 36)), 40
    ref = _mk(v, ages, 0)
    spec = _spec(ref)
    hist = ensemble.run_ensemble(v, seeds, days, age_counts=ages, concurrent=6)
    got = ensemble.run_ensemble(v, seeds, days, age_counts=ages, concurrent=6, summary=spec)   # chunks of 6, 6, 4: members apart
    su.assert_words(got.words, sm.summarise_numpy(hist, ref.nr_ages, spec, ctx=ref), got.layout)
    assert got.members == seeds


def test_branches_with_a_summary_equal_the_summary_of_their_history():
    v, ages = small_scenario()
    seeds, days = list(range(16)), 40
    past = _mk(v, ages, 2)
    past.run(20)
    snap = past.snapshot()
    spec = _spec(past)
    hist, a = ensemble.run_branches(snap, v, seeds, days, age_counts=ages)
    got, b = ensemble.run_branches(snap, v, seeds, days, age_counts=ages, summary=spec)
    su.assert_words(got.words, sm.summarise_numpy(hist, past.nr_ages, spec, ctx=past), got.layout)
    assert np.array_equal(_finals(a), _finals(b)) and got.start_day == 20
