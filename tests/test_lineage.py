"""Lineage reports on the CPU: the numpy specification (reina_model_amd/lineage.py) against a plain per-agent walker on
synthetic states, a hand-made forest with its tables written out, a simulated run on oracle B tied to the tree report and the
log report of the same state, the header against the module, and the refusals.  Every comparison is of integers and exact."""
import os
import re

import numpy as np
import pytest

import lineage_util as lu
import par_backend
import tx_util
import txlog_util as tu
from filter_util import small_scenario
from reina_model_amd import engine as eng
from reina_model_amd import ensemble, lineage as lin, simulation, txlog as txl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- 1. report_numpy == walker

def _spec_and_walk(hot, inf, cnt, log, period_days, n_periods, kind='default', max_depth=None):
    n = len(hot)
    age_start, g = tx_util.age_start_of(n), tx_util.groups(kind)
    r = lin.report_numpy(hot, inf, cnt, log, age_start, g, period_days, n_periods, max_depth)
    lu.assert_words(r.words, lu.walk_report(hot, inf, log, age_start, [int(x) for x in g], period_days, n_periods,
                                            n if max_depth is None else max_depth))
    return r


@pytest.mark.parametrize('periods', lu.PERIODS, ids=lambda p: '%dx%d' % p)
@pytest.mark.parametrize('n', tu.SIZES)
@pytest.mark.parametrize('pattern', tx_util.PATTERNS)
def test_spec_equals_walker_on_forests(pattern, n, periods):
    hot, inf, cnt, log = tu.forest_state(n, pattern)
    r = _spec_and_walk(hot, inf, cnt, log, *periods, kind='fine' if n % 2 else 'default')
    assert r.unconverged == 0 and r.trees == r.roots + r.bad_links
    if pattern == 'chain' and n > 100:
        r = _spec_and_walk(hot, inf, cnt, log, *periods, max_depth=37)       # 6 rounds: 63 links are resolved
        assert r.rounds == 6 and r.unconverged == n - 64 and r.largest_tree == 64


def test_spec_equals_walker_on_every_code_combination():
    hot, inf, cnt, log = tu.combos_state()
    for periods in lu.PERIODS:
        r = _spec_and_walk(hot, inf, cnt, log, *periods)
        assert r.bad_links == 1 and r.undated > 0 and r.links >= 81


def test_a_cycle_of_links_is_unconverged_and_counts_in_no_tree():
    hot, inf, cnt, log = lu.cycle_state()
    for depth in (None, 3):
        r = _spec_and_walk(hot, inf, cnt, log, 7, 3, max_depth=depth)
        assert r.infected == 5 and r.links == 4 and r.roots == 1 and r.bad_links == 0
        assert r.unconverged == 3 and r.trees == 1 and r.largest_tree == 2 and r.largest_root == 1
        assert int(r.lineage.sum()) == int(r.seed[:, 2].sum()) == 2 and int(r.cohort[..., 0].sum()) == 5


# ---------------------------------------------------------------------------------------------- 2. a hand-made forest

def test_hand_made_forest():
    """12 agents in three ages of four (groups 0, 1, 2), period 7 days, 4 periods (class 4: before / undated / out of range):
         0 root t=3 recovered;  1 <- 0 t=8 recovered;  4 <- 0 t=10 ill;  5 <- 4 t=15 incubating       (a tree of 4, seeded in period 0)
         2 root BEFORE recovered;  8 <- 2 t=2 recovered                                               (wholly removed, seed class 4)
         9 <- 10 (susceptible: a bad link) t=20 ill                                                   (heads a tree of its own)
         6 root t=1 dead                                                                              (wholly removed)
         11 root t=100 (beyond the range) incubating;  3, 7, 10 susceptible (3 with a stray log word)"""
    N_, B_ = txl.NONE, txl.BEFORE
    n = 12
    hot = np.zeros(n, dtype=np.uint32)
    inf = np.full(n, -1, dtype=np.int32)
    log = np.full(n, N_ << 16 | N_, dtype=np.uint32)
    for i, state, src, t in ((0, 5, -1, 3), (1, 5, 0, 8), (4, 2, 0, 10), (5, 1, 4, 15), (2, 5, -1, B_), (8, 5, 2, 2), (9, 2, 10, 20),
                             (6, 6, -1, 1), (11, 1, -1, 100)):
        hot[i], inf[i], log[i] = state | (i % 4) << 8, src, N_ << 16 | t
    log[3] = 5 << 16 | 4
    age_start = np.array([0, 4, 8, 12], dtype=np.int64)
    groups = [0, 1, 2]
    r = lin.report_numpy(hot, inf, np.zeros(n, dtype=np.int32), log, age_start, groups, 7, 4)
    lu.assert_words(r.words, lu.walk_report(hot, inf, log, age_start, groups, 7, 4, n))
    assert (r.infected, r.links, r.bad_links, r.roots, r.trees, r.unconverged) == (9, 4, 1, 4, 5, 0)
    assert (r.rounds, r.alive_agents, r.alive_trees, r.largest_tree, r.largest_root, r.undated) == (4, 4, 3, 4, 0, 2)
    Z = lambda *shape: np.zeros(shape, dtype=np.uint64)
    seed = Z(5, 4)
    seed[0], seed[2], seed[4] = (2, 1, 5, 2), (1, 1, 1, 1), (2, 1, 3, 1)
    sizes = Z(5, 33)
    sizes[0, 2] = sizes[0, 0] = sizes[2, 0] = sizes[4, 1] = sizes[4, 0] = 1
    cohort = Z(5, 16, 2)
    for p, g, removed in ((0, 0, 1), (0, 1, 1), (0, 2, 1), (1, 0, 1), (1, 1, 0), (2, 1, 0), (2, 2, 0), (4, 0, 1), (4, 2, 0)):
        cohort[p, g] = (1, removed)
    lineage = Z(5, 5)
    lineage[0, :3] = (2, 2, 1)
    lineage[2, 2] = 1
    lineage[4, 0], lineage[4, 4] = 1, 2
    mix_t, mix_c = Z(5, 16, 16), Z(5, 16, 16)
    mix_t[1, 0, 0] = mix_t[1, 0, 1] = mix_t[2, 1, 1] = mix_t[0, 0, 2] = 1
    mix_c[0, 0, 0] = mix_c[0, 0, 1] = mix_c[1, 1, 1] = mix_c[4, 0, 2] = 1
    for name, want in (('seed', seed), ('tree_sizes', sizes), ('cohort', cohort), ('lineage', lineage), ('mixing_t', mix_t),
                       ('mixing_c', mix_c)):
        assert np.array_equal(getattr(r, name), want), name
    # what is derived on the host
    r.group_labels = ['young', 'adult', 'old']
    assert r.n_groups == 3 and r.mixing_frame(1).loc['young', 'adult'] == 1 and r.mixing_frame(0, by='cohort').values.sum() == 2
    k = r.next_generation_matrix(0)
    assert k.shape == (3, 3) and k[0, 0] == 1.0 and k[0, 1] == 1.0 and k[1, 0] == 0.0
    rn = r.reproduction_number()
    assert list(rn.columns) == ['r', 'cohort', 'closed_share'] and len(rn) == 4
    assert rn['r'].iloc[0] == pytest.approx(1.0) and rn['cohort'].iloc[0] == 3 and rn['closed_share'].iloc[0] == 1.0
    assert rn['r'].iloc[1] == pytest.approx(1.0) and rn['r'].iloc[2] == 0.0 and rn['closed_share'].iloc[1] == 0.5 and np.isnan(rn['r'].iloc[3]) and rn['cohort'].iloc[3] == 0
    f = r.lineage_frame()
    assert f.shape == (5, 5) and f.index[-1] == 'before' and f.loc['before', 0] == 1 and f.loc[0, 7] == 2
    share = r.lineage_share()
    assert share.loc[0, 0] == 2 / 3 and share.loc['before', 0] == 1 / 3 and np.isnan(share.loc[0, 21])
    intro = r.introductions()
    assert list(intro.loc[0]) == [2, 1, 5, 2, 0.5] and np.isnan(intro.loc[7, 'extinct_share']) and intro.loc['before', 'extinct_share'] == 0.5
    assert r.tree_size_frame().loc[0, 4] == 1 and int(r.tree_size_frame().values.sum()) == 5
    with pytest.raises(ValueError):
        r.mixing_frame(0, by='day')
    assert r == lin.LineageReport(r.words.copy(), 7, 4, 3) and r != lin.LineageReport(r.words.copy(), 8, 4, 3)


# ---------------------------------------------------------------------------------------------- 3. a simulated run on oracle B

def _oracle(v, ages, seed):
    return simulation.make_context(v, age_counts=ages, seed=seed, ipc='auto', engine_factory=par_backend.par_engine_factory)


@pytest.fixture(scope='module')
def mini_200():
    v, ages = small_scenario()
    ctx = _oracle(v, ages, 3)
    txl.run_host_driven(ctx, 200)
    return ctx


def test_mini_population_200_days_on_oracle_b(mini_200):
    ctx = mini_200
    log = ctx.transmission_log
    assert not log.on_device
    r = log.lineage_report(period=7)
    assert r.n_periods == 29 and r.period_days == 7
    hot, inf, cnt = tu.host_state(ctx)
    table = ctx._tx_groups(None)[0]
    assert r == lin.report_numpy(hot, inf, cnt, log.words(), ctx.age_start, table, 7, 29, 201)
    # (what the engine gives on this scenario: seed 3, 200 days)
    assert (r.infected, r.roots, r.trees, r.alive_trees, r.largest_tree) == (11605, 1004, 1004, 343, 840)
    lu.assert_run_invariants(r, ctx.transmission_report(), log.report())
    assert r.rounds == 8 and r.undated == 0
    rn = r.reproduction_number()
    assert len(rn) == 29 and int(rn['cohort'].sum()) == r.infected and rn['r'].notna().sum() > 10
    assert int(r.introductions()['trees'].sum()) == r.trees
    # other periods of the same state; one list of reports through the ensemble's entry point
    for period, n_periods in ((1, None), (30, 3), (400, 1)):
        got = log.lineage_report(period, n_periods)
        assert got == lin.report_numpy(hot, inf, cnt, log.words(), ctx.age_start, table, period, got.n_periods, 201)
        assert int(got.lineage.sum()) == r.infected
    assert log.lineage_report(1).n_periods == 200 and log.lineage_report(30, 3).undated > 0
    assert ensemble.lineage_reports([ctx], period=7)[0] == r


# ---------------------------------------------------------------------------------------------- 4. the header, the library

def _header():
    with open(os.path.join(ROOT, 'include', 'reina_lineage.h')) as fh:
        return fh.read()


def test_header_constants_and_offsets_equal_the_module():
    h = _header()
    defs = dict(re.findall(r'#define (REINA_LINEAGE_\w+) (.+?)(?:\s+/\*.*)?$', h, re.M))
    env = {'REINA_LINEAGE_S_NR': int(re.search(r'REINA_LINEAGE_S_NR = (\d+)', h).group(1))}
    for name, expr in defs.items():
        env[name] = eval(re.sub(r'\b(0x[0-9A-Fa-f]+|\d+)u\b', r'\1', expr), {}, env)
    assert env['REINA_LINEAGE_VERSION'] == lin.LINEAGE_VERSION == 1
    for c, v in (('MAX_PERIODS', lin.MAX_PERIODS), ('MAX_GROUPS', lin.MAX_GROUPS), ('SIZE_BINS', lin.SIZE_BINS),
                 ('SEED_FIELDS', lin.SEED_FIELDS), ('COHORT_FIELDS', lin.COHORT_FIELDS), ('SCALARS', lin.SCALARS), ('S_NR', lin.S_NR)):
        assert env['REINA_LINEAGE_' + c] == v, c
    # the macros with an argument
    macros = dict(re.findall(r'#define (REINA_LINEAGE_\w+)\(\w+\) (.+?)(?:\s+/\*.*)?$', h, re.M))
    table = (('SEED', lin.seed_offset), ('TREE_SIZES', lin.tree_sizes_offset), ('COHORT', lin.cohort_offset), ('LINEAGE', lin.lineage_offset),
             ('MIXING_T', lin.mixing_t_offset), ('MIXING_C', lin.mixing_c_offset), ('REPORT_WORDS', lin.report_words))
    for P in (1, 53, lin.MAX_PERIODS):
        fn = {}
        for name, f in table:
            e = macros['REINA_LINEAGE_' + name].replace('(size_t)', '')
            e = re.sub(r'(REINA_LINEAGE_\w+)\(P\)', lambda m: str(fn[m.group(1)]), e)
            fn['REINA_LINEAGE_' + name] = eval(re.sub(r'\b(\d+)u\b', r'\1', e), dict(P=P), env)
            assert fn['REINA_LINEAGE_' + name] == f(P), (name, P)
        assert lin.report_words(P) == 16 + (P + 1) * (4 + 33 + 32 + (P + 1) + 512)
    assert lin.report_words(53) * 8 == 274448
    e = re.sub(r'\b(\d+)u\b', r'\1', macros['REINA_LINEAGE_SCRATCH_BYTES'].replace('(size_t)', ''))
    for n in (1, 10, 11, 12345):
        assert eval(e, dict(n_agents=n), env) == lin.scratch_bytes(n) >= 24 * n and lin.scratch_bytes(n) % 256 == 0
    enum = re.search(r'enum \{(.*?)\};', h, re.S).group(1)
    names = [re.sub(r'\s*=.*', '', x).strip() for x in re.sub(r'/\*.*?\*/', '', enum, flags=re.S).split(',')]
    names = [x for x in names if x]
    assert names[:len(lin.SCALAR_NAMES)] == ['REINA_LINEAGE_S_' + s.upper() for s in lin.SCALAR_NAMES]
    assert names[-1] == 'REINA_LINEAGE_S_NR' and len(lin.SCALAR_NAMES) <= lin.S_NR


def test_library_exports_every_function_the_header_declares():
    from reina_model_amd import build, transmission as tx
    text = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    declared = sorted(set(re.findall(r'\b(reina_[a-z_]+)\s*\(', text)))
    assert declared == sorted('reina_' + f for f in lin.LINEAGE_FUNCTIONS)
    build.build()
    lib = eng.load_hip_library()
    for fn in declared:
        assert hasattr(lib, fn), fn
    f = lin.bind_lineage_abi(lib, 'reina_')
    assert f is not None and f['lineage_version']() == lin.LINEAGE_VERSION
    # nothing else moved
    assert eng.bind_abi(lib, 'reina_')['abi_version']() == 7
    assert tx.bind_tx_abi(lib, 'reina_')['tx_version']() == 1 and txl.bind_txlog_abi(lib, 'reina_')['txlog_version']() == 1
    assert lin.bind_lineage_abi(par_backend.lib(), 'par_') is None


# ---------------------------------------------------------------------------------------------- 5. refusals, the empty state

def test_value_errors_and_the_empty_state(mini_200):
    n = 600
    hot, inf, cnt = tx_util.forest(n, 'empty')
    log = np.full(n, txl.NONE << 16 | txl.NONE, dtype=np.uint32)
    r = _spec_and_walk(hot, inf, cnt, log, 7, 10)
    assert (r.infected, r.links, r.trees, r.unconverged, r.alive_trees, r.largest_tree, r.undated) == (0,) * 7
    assert r.rounds == 10 and r.largest_root == -1 and r.largest_key == 0
    assert not r.words[lin.S_NR:].any()
    assert r.reproduction_number()['r'].isna().all() and r.lineage_share().isna().all().all()
    assert r.introductions()['extinct_share'].isna().all() and int(r.tree_size_frame().values.sum()) == 0
    assert r.mixing_frame(3).values.sum() == 0 and np.isnan(r.next_generation_matrix(3)).all()
    age_start, g = tx_util.age_start_of(n), tx_util.groups()
    for period_days, n_periods in ((0, 5), (eng.MAX_DAYS + 1, 5), (7, 0), (7, lin.MAX_PERIODS + 1)):
        with pytest.raises(ValueError):
            lin.report_numpy(hot, inf, cnt, log, age_start, g, period_days, n_periods)
    with pytest.raises(ValueError):
        lin.report_numpy(hot, inf, cnt, log, age_start, np.full(101, 16), 7, 5)
    with pytest.raises(ValueError):
        lin.LineageReport(np.zeros(17, dtype=np.uint64), 7, 5)
    tlog = mini_200.transmission_log
    with pytest.raises(ValueError, match='256'):
        tlog.lineage_report(period=1, n_periods=257)
    with pytest.raises(ValueError):
        tlog.lineage_report(period=0)
    with pytest.raises(ValueError):
        tlog.lineage_report(period=7, n_periods=0)
    with pytest.raises(ValueError, match='no transmission log'):
        v, ages = small_scenario()
        ensemble.lineage_reports([_oracle(v, ages, 1)])
    long_run = type('Ctx', (), dict(day=300, _tx_groups=mini_200._tx_groups))()
    with pytest.raises(ValueError, match='256'):
        lin._arguments(long_run, 1, None, None)      # 300 days by the day: 300 periods
