"""Transmission-tree reports on the CPU: report_numpy against a plain per-agent walker on synthetic forests, and reports of
oracle-B runs against the engine's own daily counters (reina_model_amd/transmission.py, include/reina_transmission.h)."""
import json
import os
import re

import numpy as np
import pytest

import par_backend
import snap_util
import tx_util
from reina_model_amd import engine as eng
from reina_model_amd import ensemble, simulation, transmission as tx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 511, 512, 513, 3 * 512 + 7)


def _spec_and_walk(hot, inf, cnt, n, max_depth=None, kind='default'):
    ag = tx_util.groups(kind)
    depth = n if max_depth is None else max_depth
    got = tx.report_numpy(hot, inf, cnt, tx_util.age_start_of(n), ag, depth)
    want = tx_util.walk_report(hot, inf, cnt, tx_util.age_start_of(n), ag, depth)
    return got, want


def _assert_words(got, want):
    bad = np.flatnonzero(got.words != want)
    assert not len(bad), [(int(k), int(got.words[k]), int(want[k])) for k in bad[:8]]


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('pattern', tx_util.PATTERNS)
def test_spec_equals_walker_on_forests(pattern, n):
    hot, inf, cnt = tx_util.forest(n, pattern)
    got, want = _spec_and_walk(hot, inf, cnt, n, kind='fine' if n % 2 else 'default')
    _assert_words(got, want)
    assert got.n_infected_agents == int((hot & 7 != 0).sum())


def test_spec_equals_walker_on_named_shapes():
    # one chain of 5000, a star with 10^4 infectees (bin 63 and the sums), one giant cluster
    for pattern, n, size in (('chain', 6000, 5000), ('star', 12000, 10001), ('giant', 20000, None)):
        hot, inf, cnt = tx_util.forest(n, pattern, size=size)
        got, want = _spec_and_walk(hot, inf, cnt, n)
        _assert_words(got, want)
        m = size or n
        assert got.largest_cluster == m and got.n_roots == 1 and got.unconverged == 0
        if pattern == 'chain':
            assert got.max_generation == m - 1 and got.generations.sum() == m
        if pattern == 'star':
            assert got.offspring[..., 63].sum() == 1 and got.sum_n_infected == m - 1 and got.max_generation == 1


def test_every_combination_of_variant_severity_outcome_detected_is_counted():
    hot, inf, cnt = tx_util.forest(20000, 'random', seed=3)
    got, want = _spec_and_walk(hot, inf, cnt, 20000)
    _assert_words(got, want)
    assert (got.offspring.sum(axis=-1) > 0).all()


def test_planted_bad_links_are_counted_and_shallow_depth_leaves_agents_unconverged():
    hot, inf, cnt = tx_util.forest(3000, 'bad_links', seed=1)
    got, want = _spec_and_walk(hot, inf, cnt, 3000)
    _assert_words(got, want)
    assert got.bad_links >= 4
    hot, inf, cnt = tx_util.forest(3000, 'chain', size=2000)
    got, want = _spec_and_walk(hot, inf, cnt, 3000, max_depth=5)
    _assert_words(got, want)
    assert got.rounds == 3 and got.unconverged == 2000 - 8 and got.max_generation == 7


def test_report_statistics_from_the_words():
    hot, inf, cnt = tx_util.forest(4000, 'random', seed=2)
    r = tx.report_numpy(hot, inf, cnt, tx_util.age_start_of(4000), tx_util.groups())
    inf_ = hot & 7 != 0
    sel = inf_ & (hot & 7 >= 5) & (hot & 0x400 != 0)
    n = cnt[sel].astype(np.float64)
    assert r.mean_offspring() == pytest.approx(n.mean())
    assert r.offspring_variance() == pytest.approx(n.var())
    k = r.dispersion_k()
    assert k == pytest.approx(n.mean() ** 2 / (n.var() - n.mean()))
    # the top 20 % (cut below bin 63): the infections of the 20 % largest counts
    s = np.sort(cnt[sel])[::-1]
    take = 0.2 * len(s)
    if s[int(take)] < 63:
        top = s[:int(take)].sum() + (take - int(take)) * s[int(take)]
        assert r.top_share(0.2) == pytest.approx(top / s.sum())
    assert r.top_share(1.0) == pytest.approx(1.0)
    f = r.matrix_frame()
    assert f.shape == (9, 9) and int(f.values.sum()) == r.n_linked
    back = tx.TransmissionReport.from_dict(json.loads(json.dumps(r.to_dict())))
    assert back == r and back.n_groups == r.n_groups


# ---------------------------------------------------------------------------------------------- oracle B runs
def _oracle_run(days, report_at=None):
    ctx = snap_util.make_context(20000, engine_factory=par_backend.par_engine_factory)
    hist = [ctx.run(report_at)] if report_at else []
    mid = ctx.transmission_report() if report_at else None
    hist.append(ctx.run(days - (report_at or 0)))
    return ctx, np.concatenate(hist), mid


@pytest.fixture(scope='module')
def oracle_150():
    return _oracle_run(150, report_at=60)


def test_oracle_b_report_invariants_and_counters(oracle_150):
    ctx, hist, _ = oracle_150
    assert (np.asarray(ctx.engine.tensors['hot']).view(np.uint32) & 0x4000).any(), 'contact tracing ran'
    r = ctx.transmission_report()
    assert r.n_linked == r.sum_n_infected == int(r.matrix.sum())
    assert int(r.generations.sum()) == int(r.cluster_agents.sum()) == r.n_infected_agents
    assert r.bad_links == r.unconverged == 0 and r.n_roots == int(r.clusters.sum())
    assert r.rounds == tx.rounds_for(151)
    # history row d holds the counters as day d opened, i.e. the totals of day d - 1 (row 0: the initial state, none);
    # the final counter block holds the last day's
    base = eng.C_NR * eng.MAX_AGES
    final = ctx.engine.read_counters()
    assert hist[0, base + eng.S_TOTAL_INFECTORS] == 0 and hist[0, base + eng.S_TOTAL_INFECTIONS] == 0
    infectors = int(hist[1:, base + eng.S_TOTAL_INFECTORS].sum()) + int(final[base + eng.S_TOTAL_INFECTORS])
    infections = int(hist[1:, base + eng.S_TOTAL_INFECTIONS].sum()) + int(final[base + eng.S_TOTAL_INFECTIONS])
    assert int(r.offspring[:, :, 1].sum()) == infectors
    assert int(r.offspring_sum[:, 1].sum()) == infections
    assert r.mean_offspring() == pytest.approx(infections / infectors)


def test_report_between_days_does_not_change_the_run(oracle_150):
    ctx, hist, mid = oracle_150
    plain, hist0, _ = _oracle_run(150)
    assert np.array_equal(hist, hist0)
    for name in ('hot', 'cold', 'infectees', 'counters', 'control'):
        assert np.array_equal(np.asarray(ctx.engine.tensors[name]), np.asarray(plain.engine.tensors[name])), name
    assert mid.n_infected_agents < ctx.transmission_report().n_infected_agents


def test_report_from_snapshot_equals_context_report(oracle_150):
    ctx = snap_util.make_context(20000, engine_factory=par_backend.par_engine_factory)
    ctx.run(90)
    snap = ctx.snapshot()
    want = ctx.transmission_report()
    got = tx.report_from_snapshot(snap, ctx.age_counts, ctx.age_group_indices)
    assert got == want
    with pytest.raises(ValueError):
        tx.report_from_snapshot(snap, np.roll(ctx.age_counts, 1), ctx.age_group_indices)


def test_host_ensemble_reports_are_single_reports(oracle_150):
    ctxs = [simulation.make_context(snap_util.variables(), age_counts=snap_util.population(20000), seed=s,
                                    engine_factory=par_backend.par_engine_factory) for s in (1, 7)]
    for c in ctxs:
        c.run(40)
    reps = ensemble.transmission_reports(ctxs)
    assert reps == [c.transmission_report() for c in ctxs]
    assert reps[0].group_labels == list(ctxs[0].age_group_labels)


def test_sharded_context_is_refused():
    ctx = snap_util.make_context(2000, engine_factory=par_backend.par_engine_factory)
    ctx.n_shards = 2
    with pytest.raises(ValueError):
        ctx.transmission_report()
    cfg = eng.Config()
    cfg.n_shards = 2

    class _E:
        config = cfg
    with pytest.raises(ValueError):
        tx.report_engine(_E(), tx_util.groups())


def test_failed_run_is_refused():
    ctx = snap_util.make_context(2000, engine_factory=par_backend.par_engine_factory)
    ctx.run(3)
    np.asarray(ctx.engine.tensors['counters'])[eng.C_NR * eng.MAX_AGES + eng.S_PROBLEM] = 1
    with pytest.raises(ValueError):
        ctx.transmission_report()


# ---------------------------------------------------------------------------------------------- the C header
def _header():
    with open(os.path.join(ROOT, 'include', 'reina_transmission.h')) as fh:
        return fh.read()


def test_header_constants_and_offsets_equal_the_module():
    h = _header()
    defs = dict(re.findall(r'#define (REINA_TX_\w+) (.+?)(?:\s+/\*.*)?$', h, re.M))
    env = {'REINA_TX_S_NR': int(re.search(r'REINA_TX_S_NR = (\d+)', h).group(1))}
    for name, expr in defs.items():
        if '(' in name or name == 'REINA_TX_SCRATCH_BYTES':
            continue
        e = expr.replace('u)', ')').replace('u ', ' ').replace('u*', '*')
        e = re.sub(r'(\d+)u\b', r'\1', e)
        env[name] = eval(e, {}, env)
    assert env['REINA_TX_VERSION'] == tx.TX_VERSION
    for c, v in (('VARIANTS', tx.VARIANTS), ('SEVERITIES', tx.SEVERITIES), ('OUTCOMES', tx.OUTCOMES), ('BINS', tx.BINS),
                 ('MAX_GROUPS', tx.MAX_GROUPS), ('GENERATIONS', tx.GENERATIONS), ('CLUSTER_BINS', tx.CLUSTER_BINS),
                 ('OFFSPRING', tx.OFFSPRING), ('OFFSPRING_SUM', tx.OFFSPRING_SUM), ('OFFSPRING_SUMSQ', tx.OFFSPRING_SUMSQ),
                 ('MATRIX', tx.MATRIX), ('GENERATION', tx.GENERATION), ('CLUSTERS', tx.CLUSTERS),
                 ('CLUSTER_AGENTS', tx.CLUSTER_AGENTS), ('SCALARS', tx.SCALARS)):
        assert env['REINA_TX_' + c] == v, c
    enum = re.search(r'enum \{(.*?)\};', h, re.S).group(1)
    names = [re.sub(r'\s*=.*', '', x.split('/*')[0]).strip() for x in re.sub(r'/\*.*?\*/', '', enum, flags=re.S).split(',')]
    names = [x for x in names if x]
    assert names[:len(tx.SCALAR_NAMES)] == ['REINA_TX_S_' + s.upper() for s in tx.SCALAR_NAMES]
    assert names[-1] == 'REINA_TX_S_NR' and len(tx.SCALAR_NAMES) <= tx.S_NR
    assert tx.REPORT_WORDS == tx.SCALARS + tx.S_NR == env['REINA_TX_REPORT_WORDS'] == 9834
    for n in (1, 511, 10 ** 8):
        assert tx.scratch_bytes(n) >= 20 * n and tx.scratch_bytes(n) % 256 == 0
    for fn in tx.TX_FUNCTIONS:
        assert re.search(r'\breina_%s\(' % fn, h), fn


def test_library_exports_the_report_symbols():
    from reina_model_amd import build
    build.build()
    lib = eng.load_hip_library()
    for fn in tx.TX_FUNCTIONS:
        assert hasattr(lib, 'reina_' + fn), fn
    assert tx.bind_tx_abi(lib, 'reina_') is not None
    assert tx.bind_tx_abi(par_backend.lib(), 'par_') is None
