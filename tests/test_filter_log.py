"""Logged particle filters on the CPU (include/reina_filter_log.h; reina_model_amd/filtering.py): the invariant the logs'
clone rests on, held day by day on oracle B; the kernel's delta rule against the dense copy; a cloned member with its logs
continued against a restored snapshot; the relation between the log report's incidence and the counters that the GPU test of
the whole filter relies on; weighted_band against a brute-force inverted CDF; the header against the module, and the
refusals.  Oracle B runs through par_backend, the logs host-driven.  Every comparison but weighted_band's is of integers."""
import os
import re

import numpy as np
import pytest

import course_util as cu
import par_backend
from filter_log_util import CLONE_DAY, classes, incidence_by_day
from filter_util import small_scenario, totals
from reina_model_amd import course as crs
from reina_model_amd import engine as eng
from reina_model_amd import filtering, simulation, txlog as txl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAR = par_backend.par_engine_factory
NONE_WORD = np.uint32(txl.NONE << 16 | txl.NONE)
NONE_RECORD = np.uint64((1 << 64) - 1)


def _oracle(v, ages, seed, ipc='auto', **kw):
    return simulation.make_context(v, age_counts=ages, seed=seed, ipc=ipc, engine_factory=PAR, **kw)


def _hot(ctx):
    return np.array(ctx.engine.tensors['hot']).view(np.uint32)


# ---------------------------------------------------------------------------------------------- 1. the invariant

def _assert_invariant(hot, words, records, when):
    idle = hot == 0
    assert idle.any(), when
    assert (words[idle] == NONE_WORD).all(), '%s: a log word of an agent whose hot word is 0' % when
    assert (records[idle] == NONE_RECORD).all(), '%s: a course record of an agent whose hot word is 0' % when


@pytest.mark.parametrize('ipc', ('auto', cu.IPC), ids=('plain', 'initial-condition'))
def test_hot_zero_means_all_none(ipc):
    """hot == 0 => the log word is NONE | NONE << 16 and the record four NONE: after begin and after every one of 120 days.
    (Begin and record write only where the state is not 0, and a hot word never returns to 0: the second half is asserted
    as well.)"""
    v, ages = small_scenario()
    ctx = _oracle(v, ages, 3, ipc)
    ctx.start_course_log()
    assert not ctx.transmission_log.on_device and not ctx.course_log.on_device
    _assert_invariant(_hot(ctx), ctx.transmission_log.words(), ctx.course_log.words(), 'after begin')
    seen = {'days': 0, 'hot': _hot(ctx).copy()}

    def on_day(day, hot, before, after):
        _assert_invariant(hot, ctx.transmission_log._words, after, 'after day %d' % day)
        assert (hot[seen['hot'] != 0] != 0).all(), 'day %d: a hot word returned to 0' % day
        seen['hot'] = hot.copy()
        seen['days'] += 1

    crs.run_host_driven(ctx, 120, on_day=on_day)
    assert seen['days'] == 120
    r = ctx.course_log.report()
    assert r.infected > 5000 and r.with_outcome > 1000, 'an epidemic ran'
    if ipc != 'auto':
        assert ctx.transmission_log.report().before > 0 and int(r.pathway[:, 9].sum()) > 0


# ---------------------------------------------------------------------------------------------- 2. delta == dense

@pytest.fixture(scope='module')
def two_members():
    """seeds 1 and 2 of small_scenario() at CLONE_DAY, host-driven with log and course: (contexts, histories)"""
    v, ages = small_scenario()
    ctxs = [_oracle(v, ages, sd) for sd in (1, 2)]
    return ctxs, [crs.run_host_driven(c, CLONE_DAY) for c in ctxs]


def test_delta_equals_dense(two_members):
    (src, dst), _ = two_members
    sh, dh = _hot(src), _hot(dst)
    both, src_only, dst_only, neither = classes(dh, sh)
    assert both > 0 and src_only > 0 and dst_only > 0 and neither > 0, (both, src_only, dst_only, neither)
    for s, d, dense in ((src.transmission_log.words(), dst.transmission_log.words(), filtering.clone_log_numpy),
                        (src.course_log.words(), dst.course_log.words(), filtering.clone_course_numpy)):
        assert not np.array_equal(s, d)
        want = dense(d.copy(), s)
        assert np.array_equal(want, s)
        got = filtering.clone_log_delta_numpy(d.copy(), s, dh, sh)
        assert got.dtype == d.dtype and np.array_equal(got, want)
        # the rule touches nothing where both are susceptible: with the invariant broken there, it is no dense copy
        broken = d.copy()
        idle = np.flatnonzero((sh == 0) & (dh == 0))[0]
        broken[idle] = 0
        assert filtering.clone_log_delta_numpy(broken, s, dh, sh)[idle] == 0


# ---------------------------------------------------------------------------------------------- 3. continuation on the host

def test_cloned_member_with_its_logs_continues_like_a_restored_snapshot():
    """seed a runs to `cut` with log and course; clone_state and the two dense copies into member m (which ran the same
    days under its own seed); m runs `days` more.  Reference: a fresh Context of seed m restored from a snapshot of an
    UNLOGGED run of seed a at `cut`, its logs begun and their words set to a's."""
    v, ages = small_scenario()
    seed_a, seed_m, cut, days = 31, 33, 25, 20
    a, m = _oracle(v, ages, seed_a), _oracle(v, ages, seed_m)
    for c in (a, m):
        crs.run_host_driven(c, cut)
    words_a, rec_a = a.transmission_log.words(), a.course_log.words()
    assert not np.array_equal(words_a, m.transmission_log.words()) and not np.array_equal(rec_a, m.course_log.words())
    n, mq = a.engine.config.n_agents, min(a.engine.config.max_queue, m.engine.config.max_queue)
    filtering.clone_state(filtering._host_arrays(m.engine), filtering._host_arrays(a.engine), n, mq)
    m.transmission_log.set_words(filtering.clone_log_numpy(m.transmission_log.words(), words_a))
    m.course_log.set_words(filtering.clone_course_numpy(m.course_log.words(), rec_a))
    hist = crs.run_host_driven(m, days)

    solo = _oracle(v, ages, seed_a)
    solo.run(cut)
    ref = _oracle(v, ages, seed_m, snapshot=solo.snapshot())
    ref.start_course_log()
    assert ref.course_log.begin_day == cut
    ref.transmission_log.set_words(words_a)
    ref.course_log.set_words(rec_a)
    want = crs.run_host_driven(ref, days)

    assert np.array_equal(hist, want)
    assert np.array_equal(m.transmission_log.words(), ref.transmission_log.words())
    assert np.array_equal(m.course_log.words(), ref.course_log.words())
    assert not np.array_equal(m.transmission_log.words(), words_a), 'the days after the clone were recorded'
    lr, cr = m.transmission_log.report(), m.course_log.report()
    assert np.array_equal(lr.words, ref.transmission_log.report().words) and np.array_equal(cr.words, ref.course_log.report().words)
    assert lr.before == 0 and lr.dated == lr.infected > 0, "the member's log is that of its whole ancestral path: nothing is BEFORE"
    assert lr.last_day == cut + days - 1 and lr.first_day < cut


# ---------------------------------------------------------------------------------------------- 4. incidence and the counters

def test_incidence_is_the_increment_of_all_infected(two_members):
    """The relation the GPU test of the whole filter relies on, with no shift: the agents the log dates on day d are those
    all_infected gains between history row d (before day d) and row d + 1."""
    ctxs, hists = two_members
    for ctx, hist in zip(ctxs, hists):
        inc = incidence_by_day(ctx.transmission_log.report())
        ai = totals(hist, 'all_infected')
        assert len(inc) == CLONE_DAY == len(ai)
        assert np.array_equal(inc[:-1], np.diff(ai)) and inc.sum() > 4000
        final = totals(np.asarray(ctx.engine.read_counters())[None], 'all_infected')[0]
        assert inc[-1] == final - ai[-1], 'the last day: against the final counter block'


# ---------------------------------------------------------------------------------------------- 5. weighted_band

def _result(logw):
    class Member:
        transmission_log = None
    r = filtering.FilterResult(None, [Member() for _ in logw], None, 0, '2020-02-18', 0)
    r.logw = np.asarray(logw, dtype=np.float64)
    return r


def brute_band(values, weights, q):
    """per column: the smallest finite value v at which the weight of the finite values <= v, over their total, reaches q"""
    out = np.full((values.shape[1], len(q)), np.nan)
    for d in range(values.shape[1]):
        pairs = sorted((float(x), float(w)) for x, w in zip(values[:, d], weights) if np.isfinite(x))
        total = sum(w for _, w in pairs)
        for j, x in enumerate(q):
            for v, _ in pairs:
                if sum(w for u, w in pairs if u <= v) >= x * total - 1e-12:
                    out[d, j] = v
                    break
    return out


def test_weighted_band_equals_brute_force():
    rng = np.random.default_rng(17)
    K, T = 7, 40
    q = (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0)
    for trial in range(20):
        w = rng.exponential(size=K)
        if trial % 2:
            w[rng.integers(K)] = 0.0                      # a zero weight
        with np.errstate(divide='ignore'):
            r = _result(np.log(w))
        np.testing.assert_allclose(r.weights, w / w.sum(), rtol=1e-12)
        values = rng.integers(0, 6, size=(K, T)).astype(np.float64) if trial % 3 == 0 else rng.normal(size=(K, T))   # (ties)
        values[rng.random((K, T)) < 0.2] = np.nan
        values[rng.integers(K), 1] = np.inf
        values[:, 0] = np.nan                             # a column with no finite value
        values[1:, 2] = np.nan                            # ... and one with a single finite value
        values[0, 2] = 3.5
        got = r.weighted_band(values, q)
        want = brute_band(values, r.weights, q)
        assert got.shape == (T, len(q)) and np.isnan(got[0]).all() and (got[2] == 3.5).all()
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])
        mean = r.weighted_mean(values)
        assert np.isnan(mean[0]) and (abs(mean[2] - 3.5) < 1e-12 if r.weights[0] > 0 else np.isnan(mean[2]))
        fin = np.isfinite(values[:, 5])
        np.testing.assert_allclose(mean[5], (values[fin, 5] * r.weights[fin]).sum() / r.weights[fin].sum(), rtol=1e-12)
    with pytest.raises(ValueError):
        r.weighted_band(np.zeros((K + 1, 3)))
    # equal weights: the inverted-CDF quantile of numpy
    r = _result(np.zeros(K))
    values = rng.normal(size=(K, 5))
    for j, x in enumerate((0.05, 0.5, 0.95)):
        assert np.array_equal(r.weighted_band(values, (0.05, 0.5, 0.95))[:, j], np.quantile(values, x, axis=0, method='inverted_cdf'))


# ---------------------------------------------------------------------------------------------- 6. the header, the refusals

def _header(name):
    with open(os.path.join(ROOT, 'include', name)) as fh:
        return fh.read()


def test_header_library_and_versions():
    from reina_model_amd import build
    h = _header('reina_filter_log.h')
    assert int(re.search(r'#define REINA_FILTER_LOG_VERSION (\d+)', h).group(1)) == filtering.FILTER_LOG_VERSION == 1
    text = re.sub(r'/\*.*?\*/', '', h, flags=re.S)
    declared = sorted(set(re.findall(r'\b(reina_[a-z_]+)\s*\(', text)))
    assert declared == sorted('reina_' + f for f in filtering.FILTER_LOG_FUNCTIONS)
    assert os.path.join(ROOT, 'include', 'reina_filter_log.h') in build.DEPS
    build.build()
    lib = eng.load_hip_library()
    for fn in declared:
        assert hasattr(lib, fn), fn
    f = filtering.bind_filter_log_abi(lib, 'reina_')
    assert f is not None and f['filter_log_version']() == 1
    assert filtering.bind_filter_log_abi(par_backend.lib(), 'par_') is None
    # the other headers are what they were: nothing was added to them
    assert eng.bind_abi(lib, 'reina_')['abi_version']() == 7
    assert filtering.bind_filter_abi(lib, 'reina_')['filter_version']() == filtering.FILTER_VERSION == 1
    assert txl.bind_txlog_abi(lib, 'reina_')['txlog_version']() == txl.TXLOG_VERSION == 1
    assert crs.bind_course_abi(lib, 'reina_')['course_version']() == crs.COURSE_VERSION == 1
    for name, functions in (('reina_filter.h', filtering.FILTER_FUNCTIONS), ('reina_txlog.h', txl.TXLOG_FUNCTIONS),
                            ('reina_course.h', crs.COURSE_FUNCTIONS)):
        text = re.sub(r'/\*.*?\*/', '', _header(name), flags=re.S)
        assert sorted(set(re.findall(r'\b(reina_[a-z_]+)\s*\(', text))) == sorted('reina_' + fn for fn in functions), name
    assert 'reina_group_txlog_clone' not in _header('reina_hip.h')


def test_refusals():
    v, ages = small_scenario(3000)
    for kw in (dict(txlog=True), dict(course=True)):
        with pytest.raises(eng.EngineError, match='reina_filter_log.h'):
            filtering.particle_filter(v, 2, None, days=7, engine_factory=PAR, age_counts=ages, **kw)
    # members that keep logs of their own: refused as before, alone and as a "group" of two
    a, b = _oracle(v, ages, 1, txlog=True), _oracle(v, ages, 2, txlog=True)
    plain = _oracle(v, ages, 3)
    for members in ([a], [a, b], [a, plain], [plain, a]):
        with pytest.raises(ValueError, match='transmission log'):
            filtering.FilterResult(a, members, None, 0, a.start_date, 0)
    group = eng.EngineGroup([a.engine, b.engine])
    try:
        with pytest.raises(ValueError, match='transmission log'):
            filtering.FilterResult(a, [a, b], group, 0, a.start_date, 0)
        # a logged clone on a library without the entry points
        with pytest.raises(eng.EngineError, match='reina_filter_log.h'):
            filtering.clone_group(group, [(1, 0)], log=a.transmission_log)
        before = _hot(b).copy()
        filtering.clone_group(group, [])
        assert np.array_equal(_hot(b), before)
    finally:
        group.close()
    # an unlogged result has no logged accessors
    r = filtering.particle_filter(v, 2, None, days=3, engine_factory=PAR, age_counts=ages)
    try:
        assert r.log is None
        for call in (r.log_reports, r.course_reports, r.lineage_reports, r.reproduction_number_band, r.incidence_band, r.admissions_band):
            with pytest.raises(ValueError, match='keeps no transmission log'):
                call()
    finally:
        r.close()
    with pytest.raises(ValueError, match='closed'):
        r.log_reports()
