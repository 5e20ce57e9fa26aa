"""Lineage reports on the GPU: the library's kernels (reina_lineage_report, reina_group_lineage_report) against the numpy
specification on synthetic forests and on simulated runs, against oracle B report for report, as one launch per pass for a
logged group, and between two days of a run that must not notice them.  Exact equality throughout."""
import copy
import ctypes

import numpy as np
import pytest

import lineage_util as lu
import par_backend
import snap_util
import tx_util
import txlog_util as tu
from filter_util import small_scenario
from reina_model_amd import engine as eng
from reina_model_amd import ensemble, lineage as lin, simulation, txlog as txl
from reina_model_amd.variables import VARIABLE_DEFAULTS

pytestmark = pytest.mark.gpu


def _day_word(ctx):
    return int(ctx.engine.tensors['counters'][eng.C_NR * eng.MAX_AGES + eng.S_DAY])


def _spec(ctx, period, n_periods, groups=None, words=None):
    """report_numpy of a Context's read-back state with lineage_report's depths: the day word + 1 first, every chain when
    that leaves agents unconverged"""
    hot, inf, cnt = tu.host_state(ctx)
    words = ctx.transmission_log.words() if words is None else words
    args = (hot, inf, cnt, words, ctx.age_start, ctx._tx_groups(groups)[0], period, n_periods)
    r = lin.report_numpy(*args, min(max(_day_word(ctx), 0), eng.MAX_DAYS) + 1)
    return lin.report_numpy(*args, len(hot)) if r.unconverged else r


def _synthetic_case(hot, inf, cnt, log, periods, kind='default', day=4095):
    ctx = snap_util.make_context(len(hot))
    tx_util.put_forest(ctx, hot, inf, cnt, day=day)
    tlog = ctx.start_transmission_log()
    assert tlog.on_device and ctx.engine.lineage_f is not None
    tlog.set_words(log)
    g = tx_util.groups(kind)
    got = tlog.lineage_report(periods[0], periods[1], g)
    lu.assert_words(got.words, _spec(ctx, periods[0], periods[1], g, words=log).words)
    return got


# ---------------------------------------------------------------------------------------------- 6. device == report_numpy

@pytest.mark.parametrize('n', (1, 511, 512, 513, 3 * 512 + 7))
@pytest.mark.parametrize('pattern', tx_util.PATTERNS)
def test_kernels_equal_spec_on_forests(pattern, n):
    k = tx_util.PATTERNS.index(pattern) + tu.SIZES.index(n)
    r = _synthetic_case(*tu.forest_state(n, pattern), lu.PERIODS[k % 4], kind='fine' if n % 2 else 'default')
    assert r.unconverged == 0 and r.rounds == 13


@pytest.mark.parametrize('periods', lu.PERIODS, ids=lambda p: '%dx%d' % p)
def test_kernels_equal_spec_on_every_code_combination_and_on_a_cycle(periods):
    r = _synthetic_case(*tu.combos_state(), periods)
    assert r.bad_links == 1 and r.undated > 0
    r = _synthetic_case(*lu.cycle_state(), periods)
    assert r.unconverged == 3 and r.trees == 1 and r.rounds == lin._tx.rounds_for(10)


def test_kernels_equal_spec_on_large_forests():
    n = 3_000_000
    log = tu.random_log(n)

    def case(pattern, periods, size=None):
        hot, inf, cnt = tx_util.forest(n, pattern, size=size)
        return _synthetic_case(hot, inf, cnt, log, periods)

    r = case('giant', (7, 43), size=2_000_000)          # one tree of 2e6 agents: the wave aggregation and the hash
    assert r.largest_tree == 2_000_000 and r.trees == 1
    r = case('roots', (1, 256))                         # 3e6 distinct roots: the hash's probes fail, global atomics take over
    assert r.trees == r.roots == n and r.largest_root == 0 and int(r.tree_sizes[:, 0].sum()) == n
    r = case('random', (30, 5))
    assert r.links > 10 ** 6 and r.unconverged == 0
    r = case('bad_links', (400, 1))
    assert r.bad_links > 0 and r.trees == r.roots + r.bad_links


# ---------------------------------------------------------------------------------------------- 8. the second pass

def test_deep_chain_takes_the_second_pass():
    # a chain of 5000 in an engine whose day word says 3 days have run: the first pass resolves 3 links, the second all
    hot, inf, cnt = tx_util.forest(6000, 'chain', size=5000)
    r = _synthetic_case(hot, inf, cnt, tu.random_log(6000), (7, 43), day=3)
    assert r.rounds == lin._tx.rounds_for(6000) and r.unconverged == 0 and r.largest_tree == 5000 and r.trees == 1


# ---------------------------------------------------------------------------------------------- 9. simulated runs

def _make(v, ages=None, seed=1, txlog=True, engine_factory=None):
    return simulation.make_context(v, age_counts=ages, seed=seed, ipc='auto', txlog=txlog, engine_factory=engine_factory)


def _device_report_equals_spec(ctx, period=7, n_periods=None):
    got = ctx.transmission_log.lineage_report(period, n_periods)
    lu.assert_words(got.words, _spec(ctx, period, got.n_periods).words)
    return got


def test_mini_200_days_equals_spec_and_oracle_b():
    v, ages = small_scenario()
    dev = _make(v, ages, 3)
    dev.run(200)
    assert dev.transmission_log.on_device
    r = _device_report_equals_spec(dev)
    host = _make(v, ages, 3, txlog=False, engine_factory=par_backend.par_engine_factory)
    txl.run_host_driven(host, 200)
    want = host.transmission_log.lineage_report(7)
    lu.assert_words(r.words, want.words)
    assert (r.infected, r.roots, r.trees, r.alive_trees, r.largest_tree) == (11605, 1004, 1004, 343, 840)
    _device_report_equals_spec(dev, 1)
    _device_report_equals_spec(dev, 30, 3)           # (most infections out of range: class P)
    _device_report_equals_spec(dev, eng.MAX_DAYS, 1)


def test_hus_200_days_equals_spec_and_keeps_the_invariants():
    ctx = _make(copy.deepcopy(VARIABLE_DEFAULTS), None, 5)
    ctx.run(200)
    r = _device_report_equals_spec(ctx)
    assert r.n_periods == 29 and r.infected > 300000
    lu.assert_run_invariants(r, ctx.transmission_report(), ctx.transmission_log.report())


# ---------------------------------------------------------------------------------------------- 10. a logged group

def test_a_logged_group_is_reported_by_one_launch_per_pass():
    v = snap_util.variables()
    ages = snap_util.population(20000)
    ctxs = [simulation.make_context(v, age_counts=ages, seed=s) for s in range(60, 68)]
    ensemble.run_group_plan(ctxs, ctxs[0].make_plan(120), txlog=True)
    glog = ctxs[0].transmission_log.device
    assert glog.group is not None and glog.members == 8
    # two members get synthetic states of other depths: member 1's chain outruns its day word (a second pass resolves it),
    # member 5's day word asks for more rounds than the simulated members' (a synthetic state is never stepped again)
    logs = {}
    for m, size, day in ((1, 3000, 2), (5, 900, 1000)):
        hot, inf, cnt = tx_util.forest(20000, 'chain', size=size, seed=m)
        tx_util.put_forest(ctxs[m], hot, inf, cnt, day=day)
        logs[m] = tu.random_log(20000, seed=m)
        ctxs[m].transmission_log.set_words(logs[m])
    reps = ensemble.lineage_reports(ctxs, period=7, n_periods=18)
    assert len(reps) == 8
    for m, c in enumerate(ctxs):
        lu.assert_words(reps[m].words, _spec(c, 7, 18).words)
        assert reps[m].group_labels == list(c.age_group_labels)
    assert reps[0].rounds == 7 and reps[5].rounds == 10 and reps[1].rounds == lin._tx.rounds_for(20000)
    assert reps[1].largest_tree == 3000 and reps[5].largest_tree == 900 and not any(r.unconverged for r in reps)
    assert len({r.infected for r in reps}) > 2 and all(r.links > 0 for r in reps)
    # a member's own report takes the numpy route on host copies
    assert ctxs[3].transmission_log.lineage_report(7, 18) == reps[3]


def test_a_group_takes_its_second_pass_as_a_group_and_replaces_only_the_deep_member():
    """three members of 513 agents; only member 1 holds a chain deeper than its day + 1.  Every member's words are report_numpy's
    with max_depth = n_agents, and those of members 0 and 2 are the words of their first pass.  `rounds` is one of the words, so
    both can hold only if the first pass of members 0 and 2 runs the rounds of the second: their day + 1 is 513.  The words
    then cannot tell a kept row from a replaced one; what pins the mechanism is the list of launches -- the group entry point
    twice, no member on its own"""
    n = 513
    ctxs = [snap_util.make_context(n) for _ in range(3)]
    states = [tu.forest_state(n, 'random'), tu.forest_state(n, 'chain'), tu.forest_state(n, 'bad_links', seed=2)]
    days = (n - 1, 3, n - 1)
    group = eng.EngineGroup([c.engine for c in ctxs])
    glog = txl.DeviceLog(ctxs[0].engine, group=group)
    try:
        for m, (c, (hot, inf, cnt, log), day) in enumerate(zip(ctxs, states, days)):
            tx_util.put_forest(c, hot, inf, cnt, day=day)
            c.transmission_log = txl.TransmissionLog(c, device=glog, member=m)
            c.transmission_log.set_words(log)
        f, launches = ctxs[0].engine.lineage_f, []
        for name in ('lineage_report', 'group_lineage_report'):
            f[name] = (lambda real, name: lambda *args: (launches.append(name), real(*args))[1])(f[name], name)
        g = tx_util.groups('fine')
        reps = ensemble.lineage_reports(ctxs, 7, 43, g)
    finally:
        glog.close()
        group.close()
    assert launches == ['group_lineage_report'] * 2                  # one launch per pass, no member on its own
    spec = lambda m, depth: lin.report_numpy(*states[m], ctxs[m].age_start, g, 7, 43, depth)
    for m in range(3):
        lu.assert_words(reps[m].words, spec(m, n).words)
        assert reps[m].unconverged == 0
    for m in (0, 2):
        lu.assert_words(reps[m].words, spec(m, days[m] + 1).words)
    assert spec(1, days[1] + 1).unconverged > 0 and reps[1].largest_tree == n and reps[2].bad_links > 0


# ---------------------------------------------------------------------------------------------- 11. a report changes nothing

def test_report_between_two_days_changes_nothing():
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    a, b = _make(v, None, 9), _make(v, None, 9)
    h1 = a.run(60)
    r = a.transmission_log.lineage_report()
    assert r.infected > 0 and r.n_periods == 9
    ha = np.concatenate([h1, a.run(60)])
    hb = b.run(120)
    assert np.array_equal(ha, hb)
    assert np.array_equal(a.engine.read_counters(), b.engine.read_counters())
    for name in ('hot', 'cold'):
        assert bool((a.engine.tensors[name] == b.engine.tensors[name]).all()), name
    assert np.array_equal(a.transmission_log.words(), b.transmission_log.words())


# ---------------------------------------------------------------------------------------------- 5. refusals of the library

def test_refusals():
    v, ages = small_scenario()
    c = _make(v, ages, 1)
    c.run(3)
    e, log = c.engine, c.transmission_log.device
    f, torch = e.lineage_f, e.alloc.torch
    n = e.config.n_agents
    scratch = torch.empty(lin.scratch_bytes(n) + 16, dtype=torch.uint8, device=e.alloc.device)
    rep = torch.zeros(lin.report_words(4) + 2, dtype=torch.int64, device=e.alloc.device)
    table = np.zeros(eng.MAX_AGES, dtype=np.uint8)
    call = lambda name, h, t, ng, pd, P, s, r: f[name](h, t.ctypes.data, ng, pd, P, 0, s, r, e.alloc.stream())
    one = lambda **kw: call('lineage_report', log._h, kw.get('t', table), kw.get('ng', 1), kw.get('pd', 7), kw.get('P', 4),
                            scratch.data_ptr() + kw.get('s_off', 0), rep.data_ptr() + kw.get('r_off', 0))
    assert one() == 0
    for kw, text in ((dict(pd=0), b'period_days'), (dict(pd=eng.MAX_DAYS + 1), b'period_days'), (dict(P=0), b'n_periods'),
                     (dict(P=lin.MAX_PERIODS + 1), b'n_periods'), (dict(ng=0), b'n_groups'), (dict(ng=17), b'n_groups'),
                     (dict(s_off=8), b'aligned'), (dict(r_off=8), b'aligned')):
        assert one(**kw) == -1 and text in e.f['last_error'](), kw
    bad = table.copy()
    bad[5] = 3
    assert one(t=bad, ng=3) == -1 and b'not below n_groups' in e.f['last_error']()
    # a single engine's log through the group entry point, and the other way round
    ptrs = (ctypes.c_void_p * 1)(scratch.data_ptr())
    assert call('group_lineage_report', log._h, table, 1, 7, 4, ptrs, rep.data_ptr()) == -1 and b'one engine' in e.f['last_error']()
    ctxs = [_make(v, ages, sd, txlog=False) for sd in (1, 2)]
    group = eng.EngineGroup([x.engine for x in ctxs])
    glog = txl.DeviceLog(ctxs[0].engine, group=group)
    assert call('lineage_report', glog._h, table, 1, 7, 4, scratch.data_ptr(), rep.data_ptr()) == -1 and b'group' in e.f['last_error']()
    glog.close()
    group.close()
    with pytest.raises(ValueError, match='256'):
        c.transmission_log.lineage_report(1, 257)
