"""The dated transmission log on the CPU: the numpy specification (reina_model_amd/txlog.py) against a plain per-agent walker
on synthetic states, record_numpy on hand-made hot words, simulated runs on oracle B through run_host_driven (with the facts
k_txlog_day's hot-word form relies on asserted day by day), the header against the module, and the refusals.  Every
comparison is of integers and exact."""
import copy
import os
import re

import numpy as np
import pytest

import par_backend
import tx_util
import txlog_util as tu
from filter_util import small_scenario
from reina_model_amd import engine as eng
from reina_model_amd import simulation, transmission as tx, txlog as txl
from reina_model_amd.variables import VARIABLE_DEFAULTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IPC = dict(dead=2, in_icu=1, in_ward=3, confirmed_cases=20, infected_cases=40, incubating=15, ill=10, recovered=10)   # tests/test_snapshot.py's
W = lambda onset, infection: np.uint32(onset << 16 | infection)


# ---------------------------------------------------------------------------------------------- 1. report_numpy == walker

def _spec_and_walk(hot, inf, cnt, log, n, kind='default', n_days=tu.N_DAYS):
    age_start, g = tx_util.age_start_of(n), tx_util.groups(kind)
    r = txl.report_numpy(hot, inf, cnt, log, age_start, g, n_days)
    tu.assert_words(r.words, tu.walk_report(hot, inf, cnt, log, age_start, [int(x) for x in g], n_days))
    return r


@pytest.mark.parametrize('n', tu.SIZES)
@pytest.mark.parametrize('pattern', tx_util.PATTERNS)
def test_spec_equals_walker_on_forests(pattern, n):
    hot, inf, cnt, log = tu.forest_state(n, pattern)
    _spec_and_walk(hot, inf, cnt, log, n, 'fine' if n % 2 else 'default')


def test_spec_equals_walker_on_every_code_combination_and_clipping():
    hot, inf, cnt, log = tu.combos_state()
    r = _spec_and_walk(hot, inf, cnt, log, len(hot))
    assert r.links >= 81 + 30 and r.bad_links == 1
    assert (r.link_phase.sum(axis=0) > 0).all(), 'every link phase occurs'
    assert r.generation_nonpositive >= 2, 'the planted negative and zero generation intervals are counted'
    for h in (r.incubation, r.generation, r.serial, r.tost):   # both end bins of every histogram are hit (twice: at and beyond)
        assert h.sum(axis=0)[0] >= 2 and h.sum(axis=0)[-1] >= 2
    # (known days >= 300: t = 120 + 200, o = 150 + 150, and o_s = 300, t_i = 300, o_i = 305 of the last pair)
    assert r.out_of_range == 5 and r.before > 0 and r.with_onset > 0
    # the same state with a short and with the longest range
    _spec_and_walk(hot, inf, cnt, log, len(hot), n_days=1)
    _spec_and_walk(hot, inf, cnt, log, len(hot), n_days=eng.MAX_DAYS)


def test_empty_state_and_report_accessors():
    n = 600
    hot, inf, cnt = tx_util.forest(n, 'empty')
    r = _spec_and_walk(hot, inf, cnt, np.full(n, W(txl.NONE, txl.NONE)), n)
    assert r.infected == 0 and r.first_day == -1 and r.last_day == -1 and r.presymptomatic_share() is None
    hot, inf, cnt, log = tu.combos_state()
    r = _spec_and_walk(hot, inf, cnt, log, len(hot))
    f = r.incidence_frame()
    assert f.shape == (tu.N_DAYS, r.n_groups) and int(f.values.sum()) == int(r.incidence.sum())
    assert sum(int(r.incidence_frame(v).values.sum()) for v in range(4)) == int(r.incidence.sum())
    gi = r.generation_interval()
    assert gi.total() == r.links_dated and gi.series().index[0] == 0 and gi.mean() is not None
    assert r.serial_interval().series().index[0] == -32 and r.onset_to_transmission().series().index[0] == -24
    assert r.incubation_period().total() == int(r.incubation.sum())
    p = r.link_phase.sum(axis=0)
    assert r.presymptomatic_share() == int(p[0]) / (int(p[0]) + int(p[1]))
    rc = r.case_reproduction_number()
    assert list(rc.columns) == ['r_c', 'cohort', 'closed_share'] and int(rc['cohort'].sum()) == int(r.cohort[..., 0].sum())
    day = int(np.flatnonzero(r.cohort[..., 0].sum(axis=1))[0])
    assert rc['r_c'].iloc[day] == r.cohort[day, :, 1].sum() / r.cohort[day, :, 0].sum()


@pytest.mark.parametrize('pattern', tx_util.PATTERNS)
def test_tree_report_and_log_report_classify_links_alike(pattern):
    # the two specifications on one state (the device twin: tests/test_transmission_gpu.py)
    n = 513
    hot, inf, cnt, log = tu.forest_state(n, pattern)
    age_start, g = tx_util.age_start_of(n), tx_util.groups()
    tree = tx.report_numpy(hot, inf, cnt, age_start, g, n)
    tu.assert_same_links(tree, txl.report_numpy(hot, inf, cnt, log, age_start, g, tu.N_DAYS))
    if pattern == 'bad_links':
        assert tree.bad_links > 0 and tree.n_linked > 0 and tree.n_roots > 0


# ---------------------------------------------------------------------------------------------- 2. record_numpy

def test_begin_and_record_on_hand_made_hot_words():
    S = lambda st, hi=0: np.uint32(st | hi << 24 | 0x8000)
    hot = np.array([0, S(1), S(2), S(3), S(4), S(5), S(6)], dtype=np.uint32)
    log = txl.begin_numpy(hot)
    B, N = txl.BEFORE, txl.NONE
    assert list(log) == [W(N, N), W(N, B), W(B, B), W(B, B), W(B, B), W(B, B), W(B, B)]
    # day 7: nothing changes on a state that the begin pass has seen (BEFORE is never overwritten)
    assert np.array_equal(txl.record_numpy(log, hot, 7), log)
    # every transition from NONE
    log = np.full(8, W(N, N), dtype=np.uint32)
    hot = np.array([0, S(1), S(2), S(3), S(4), S(5), S(6), 0], dtype=np.uint32)
    got = txl.record_numpy(log, hot, 9)
    assert list(got) == [W(N, N), W(N, 9), W(9, 9), W(9, 9), W(9, 9), W(9, 9), W(9, 9), W(N, N)]
    # incubating since day 9 falls ill on day 12: the infection day stays, the onset is dated; later days change nothing
    hot2 = hot.copy()
    hot2[1] = S(2)
    hot2[7] = S(1)
    got2 = txl.record_numpy(got, hot2, 12)
    assert got2[1] == W(12, 9) and got2[7] == W(N, 12) and np.array_equal(got2[2:7], got[2:7]) and got2[0] == W(N, N)
    hot3 = hot2.copy()
    hot3[1] = S(5)
    hot3[7] = S(5)          # recovered without ever being seen ill: dated as an onset on the day it is first seen removed
    got3 = txl.record_numpy(got2, hot3, 20)
    assert got3[1] == W(12, 9) and got3[7] == W(20, 12)
    # an agent incubating before the log began keeps BEFORE and gets a dated onset
    log = txl.begin_numpy(np.array([S(1)], dtype=np.uint32))
    got = txl.record_numpy(log, np.array([S(2)], dtype=np.uint32), 3)
    assert got[0] == W(3, B)
    with pytest.raises(ValueError):
        txl.record_numpy(log, hot[:1], eng.MAX_DAYS)
    assert got.dtype == np.uint32


# ---------------------------------------------------------------------------------------------- 3. simulated runs on oracle B

def _oracle(v, ages, seed, ipc='auto', txlog=False):
    return simulation.make_context(v, age_counts=ages, seed=seed, ipc=ipc, engine_factory=par_backend.par_engine_factory, txlog=txlog)


def _check_run(ctx, hist, facts, equality):
    """the per-day and whole-run facts of a host-driven logged run"""
    final = ctx.engine.read_counters()
    counted = tu.new_infections(hist, final)
    imports = tu.pre_init_imports(ctx)
    d0 = ctx.day - len(hist)
    for k in range(len(hist)):
        extra = facts.dated[d0 + k] - int(counted[k])
        assert 0 <= extra <= imports.get(d0 + k, 0), (d0 + k, facts.dated[d0 + k], int(counted[k]), imports.get(d0 + k, 0))
        if equality:
            assert extra == imports.get(d0 + k, 0), (d0 + k, extra)
    log = ctx.transmission_log
    r = log.report()
    assert r == tu.spec_report(ctx, log.words())
    hot, inf, cnt = tu.host_state(ctx)
    words = log.words()
    t = words & 0xFFFF
    assert r.generation_nonpositive == 0 and r.bad_links == 0 and r.out_of_range == 0
    assert int(r.incidence.sum()) == r.dated == sum(facts.dated.values())
    assert int(r.onsets.sum()) == r.with_onset == sum(facts.onsets.values())
    linked = np.flatnonzero(((hot & 7) != 0) & (inf >= 0))
    assert int(r.cohort[..., 1].sum()) == int((t[inf[linked]] < txl.BEFORE).sum()), 'sum of n_infected of dated agents == links whose infector is dated'
    assert int(r.cohort[..., 0].sum()) == r.dated and r.links == len(linked)
    assert r.infected == r.dated + r.before
    return r


@pytest.fixture(scope='module')
def mini_200():
    v, ages = small_scenario()
    ctx = _oracle(v, ages, 3)
    facts = tu.DayFacts()
    hist = txl.run_host_driven(ctx, 200, on_day=facts)
    return ctx, hist, facts


def test_mini_population_200_days_facts(mini_200):
    ctx, hist, facts = mini_200
    r = _check_run(ctx, hist, facts, equality=False)
    assert r.dated > 5000 and r.before == 0 and r.first_day >= 0 and r.last_day <= 199
    gi, inc = r.generation_interval(), r.incubation_period()
    assert gi.counts[0] == 0 and gi.total() == r.links_dated > 0 and 3 < gi.mean() < 8
    assert inc.counts[0] == 0 and inc.total() == r.with_onset
    assert 0.2 < r.presymptomatic_share() < 0.7
    assert int(r.link_phase[:, 3].sum()) == 0, 'no link involves BEFORE in a run logged from the start without an initial condition'
    ll = ctx.transmission_log.line_list()
    assert len(ll) == r.infected and (ll['infection_day'] >= 0).all()
    k = ll[ll['infector'] >= 0]
    by = ll.set_index('agent')['infection_day']
    assert (k['infection_day'].values > by.loc[k['infector'].values].values).all()


def test_context_route_on_oracle_b_equals_run_host_driven(mini_200):
    ctx, hist, _ = mini_200
    v, ages = small_scenario()
    c = _oracle(v, ages, 3, txlog=True)
    assert c.transmission_log is not None and not c.transmission_log.on_device
    h1 = c.run(120)                      # run() takes the host-driven route on a library without the entry points
    for _ in range(80):                  # ... and iterate() records too
        c.iterate()
    assert np.array_equal(h1, hist[:120])
    assert np.array_equal(c.transmission_log.words(), ctx.transmission_log.words())
    plain = _oracle(v, ages, 3)
    assert np.array_equal(plain.run(200), hist), 'a logged run computes what a plain run computes'


def test_initial_condition_is_before_and_its_incubating_agents_get_dated_onsets():
    v, ages = small_scenario()
    ctx = _oracle(v, ages, 5, ipc=IPC, txlog=True)
    hot0 = np.array(ctx.engine.tensors['hot']).view(np.uint32)
    begin = ctx.transmission_log.words()
    placed = np.flatnonzero(hot0 & 7)
    assert np.array_equal(np.flatnonzero((begin & 0xFFFF) == txl.BEFORE), placed) and ((begin & 0xFFFF)[hot0 & 7 == 0] == txl.NONE).all()
    incubating = np.flatnonzero((hot0 & 7) == 1)
    assert len(incubating) == IPC['incubating'] and ((hot0[incubating] >> 24) == 0).all(), 'they carry day 0 in bits 24-31: the trap of day 0'
    assert ((begin >> 16)[incubating] == txl.NONE).all() and ((begin >> 16)[np.flatnonzero((hot0 & 7) >= 2)] == txl.BEFORE).all()
    assert ((hot0[placed] & tu.ACTIVE) != 0).all()
    facts = tu.DayFacts()
    hist = txl.run_host_driven(ctx, 120, on_day=facts)
    r = _check_run(ctx, hist, facts, equality=False)
    end = ctx.transmission_log.words()
    assert np.array_equal(np.flatnonzero((end & 0xFFFF) == txl.BEFORE), placed), 'exactly the placed agents are BEFORE'
    assert r.before == len(placed) and ((end >> 16)[incubating] < 120).all(), 'the incubating ones got a dated onset'
    assert r.dated > 5000


@pytest.mark.slow
def test_hus_120_days_facts_and_import_batches():
    ctx = _oracle(copy.deepcopy(VARIABLE_DEFAULTS), None, 5, ipc=None)
    facts = tu.DayFacts()
    hist = txl.run_host_driven(ctx, 120, on_day=facts)
    r = _check_run(ctx, hist, facts, equality=True)
    imports = tu.pre_init_imports(ctx)
    assert sum(x for d, x in imports.items() if d < 120) > 0
    assert r.dated > 100000


def test_start_mid_run_marks_the_past_before(mini_200):
    ctx, hist, _ = mini_200
    v, ages = small_scenario()
    c = _oracle(v, ages, 3)
    c.run(60)
    c.start_transmission_log()
    h2 = c.run(140)
    assert np.array_equal(h2, hist[60:])
    full, part = ctx.transmission_log.words(), c.transmission_log.words()
    ft, fo, pt, po = full & 0xFFFF, full >> 16, part & 0xFFFF, part >> 16
    assert np.array_equal(pt, np.where(ft < 60, txl.BEFORE, ft)) and np.array_equal(po, np.where(fo < 60, txl.BEFORE, fo))
    assert c.transmission_log.begin_day == 60


# ---------------------------------------------------------------------------------------------- 4. the header, the library

def _header():
    with open(os.path.join(ROOT, 'include', 'reina_txlog.h')) as fh:
        return fh.read()


def test_header_constants_and_offsets_equal_the_module():
    h = _header()
    defs = dict(re.findall(r'#define (REINA_TXLOG_\w+) (.+?)(?:\s+/\*.*)?$', h, re.M))
    env = {'REINA_TXLOG_S_NR': int(re.search(r'REINA_TXLOG_S_NR = (\d+)', h).group(1))}
    for name, expr in defs.items():
        e = re.sub(r'\b(0x[0-9A-Fa-f]+|\d+)u\b', r'\1', expr)
        env[name] = eval(e, {}, env)
    assert env['REINA_TXLOG_VERSION'] == txl.TXLOG_VERSION
    for c, v in (('NONE', txl.NONE), ('BEFORE', txl.BEFORE), ('VARIANTS', txl.VARIANTS), ('MAX_GROUPS', txl.MAX_GROUPS),
                 ('INCUBATION_BINS', txl.INCUBATION_BINS), ('GENERATION_BINS', txl.GENERATION_BINS), ('SERIAL_BINS', txl.SERIAL_BINS),
                 ('SERIAL_SHIFT', txl.SERIAL_SHIFT), ('TOST_BINS', txl.TOST_BINS), ('TOST_SHIFT', txl.TOST_SHIFT), ('PHASES', txl.PHASES),
                 ('COHORT_FIELDS', txl.COHORT_FIELDS), ('INCUBATION', txl.INCUBATION), ('GENERATION', txl.GENERATION),
                 ('SERIAL', txl.SERIAL), ('TOST', txl.TOST), ('LINK_PHASE', txl.LINK_PHASE), ('SCALARS', txl.SCALARS),
                 ('FIXED_WORDS', txl.FIXED_WORDS), ('DAY_WORDS', txl.DAY_WORDS)):
        assert env['REINA_TXLOG_' + c] == v, c
    assert txl.DAY_WORDS == 80 and txl.BEFORE > eng.MAX_DAYS
    # the macros with an argument
    macros = dict(re.findall(r'#define (REINA_TXLOG_\w+)\(n_days\) (.+?)(?:\s+/\*.*)?$', h, re.M))
    for n_days in (1, 365, eng.MAX_DAYS):
        fn = {}
        for name in ('REINA_TXLOG_INCIDENCE', 'REINA_TXLOG_ONSETS', 'REINA_TXLOG_COHORT', 'REINA_TXLOG_REPORT_WORDS'):
            e = macros[name].replace('(size_t)', '')
            e = re.sub(r'(REINA_TXLOG_\w+)\(n_days\)', lambda m: str(fn[m.group(1)]), e)
            fn[name] = eval(e, dict(n_days=n_days), env)
        assert fn['REINA_TXLOG_INCIDENCE'] == txl.incidence_offset(n_days) and fn['REINA_TXLOG_ONSETS'] == txl.onsets_offset(n_days)
        assert fn['REINA_TXLOG_COHORT'] == txl.cohort_offset(n_days) and fn['REINA_TXLOG_REPORT_WORDS'] == txl.report_words(n_days)
    assert txl.report_words(365) * 8 < 250_000
    enum = re.search(r'enum \{(.*?)\};', h, re.S).group(1)
    names = [re.sub(r'\s*=.*', '', x).strip() for x in re.sub(r'/\*.*?\*/', '', enum, flags=re.S).split(',')]
    names = [x for x in names if x]
    assert names[:len(txl.SCALAR_NAMES)] == ['REINA_TXLOG_S_' + s.upper() for s in txl.SCALAR_NAMES]
    assert names[-1] == 'REINA_TXLOG_S_NR' and len(txl.SCALAR_NAMES) <= txl.S_NR


def _declared_functions():
    text = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    return sorted(set(re.findall(r'\b(reina_[a-z_]+)\s*\(', text)))


def test_library_exports_every_function_the_header_declares():
    from reina_model_amd import build
    assert _declared_functions() == sorted('reina_' + f for f in txl.TXLOG_FUNCTIONS)
    build.build()
    lib = eng.load_hip_library()
    for fn in _declared_functions():
        assert hasattr(lib, fn), fn
    f = txl.bind_txlog_abi(lib, 'reina_')
    assert f is not None and f['txlog_version']() == txl.TXLOG_VERSION == 1
    assert eng.bind_abi(lib, 'reina_')['abi_version']() == 7
    assert txl.bind_txlog_abi(par_backend.lib(), 'par_') is None


# ---------------------------------------------------------------------------------------------- 10. refusals (host side)

def test_refusals_on_the_host():
    from reina_model_amd import filtering, policy as pol
    v, ages = small_scenario()
    sharded = _oracle(v, ages, 1)
    sharded.n_shards = 2
    with pytest.raises(ValueError, match='sharded'):
        sharded.start_transmission_log()
    assert sharded.transmission_log is None
    c = _oracle(v, ages, 1, txlog=True)
    with pytest.raises(ValueError, match='transmission log'):
        c.snapshot()
    with pytest.raises(ValueError, match='already'):
        c.start_transmission_log()
    with pytest.raises(ValueError, match='transmission log'):
        filtering.FilterResult(c, [c], None, 0, c.start_date, 0)
    p = pol.Policy(pol.Signal('dead'), levels=[[], [['limit-mobility', 30]]], up=[2 ** 31 - 1], down=[0])
    with pytest.raises(ValueError, match='policy'):
        simulation.make_context(v, age_counts=ages, seed=1, ipc=None, engine_factory=par_backend.par_engine_factory, policy=p, txlog=True)
    plain = _oracle(v, ages, 1)
    snap = plain.snapshot()
    with pytest.raises(ValueError, match='transmission log'):
        c.restore(snap)
    with pytest.raises(ValueError):
        c.transmission_log.report(n_days=eng.MAX_DAYS + 1)
