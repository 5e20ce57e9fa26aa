"""The plan of a day's launches (reina_model_amd/csrc/reina_launch.h: plan_day) on the CPU: the header compiled alone by the
host compiler behind a small extern "C" shim, as tests/par_backend.py compiles oracle B, and called through ctypes.

Results do not depend on launch geometry -- the parity suite proves that -- so a wrong grid passes every test of results and
shows up only as speed, at sizes no GPU test runs (10^8 agents, groups of 128).  Two kinds of check here:

  * recorded: tests/test_launch_plan.json holds the full DayPlan of a case grid, written by
    `python tests/test_launch_plan.py --record`.  It was recorded only after the launches of this header's first version had
    been found identical to those of the arithmetic it replaced (parent commit 76c0a42), dispatch by dispatch -- kernel, grid,
    workgroup size, LDS size, in order -- on the cases of tools/launch_trace.py under the kernel trace on one MI355X
    (profiles/day_plan_trace_ab.txt), and the cases of the grid that trace reaches (TRACED below) were checked to carry the
    grids the trace shows.  A change of a recorded value is a change of launch geometry: trace it again before recording.
  * asserted from the comments of the code itself, on every case of the grid: the bounds below.
"""
import ctypes
import itertools
import json
import os
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from reina_model_amd import engine as eng  # noqa: E402

HEADER = os.path.join(ROOT, 'reina_model_amd', 'csrc', 'reina_launch.h')
RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'test_launch_plan.json')
SHIM = r'''
#include "%s"
extern "C" {
int shim_plan_day(const LaunchShape *sh, uint32_t K, int testing_ever, uint32_t rows, uint32_t crows, const reina_day_t *dp, DayPlan *p) {
    return plan_day(*sh, K, testing_ever != 0, rows, crows, *dp, p);
}
uint32_t shim_member_cap(uint32_t n_cus, uint32_t K) { return member_cap(n_cus, K); }
uint32_t shim_lds_rows_for(const LaunchShape *sh, uint32_t rows, uint32_t room) { return lds_rows_for(*sh, rows, room); }
int shim_plan_fits_small(const LaunchShape *sh, const DayPlan *p) { return plan_fits_small(*sh, *p); }
uint32_t shim_constant(int k) {
    const uint32_t c[] = {sizeof(LaunchShape), sizeof(DayPlan), sizeof(reina_day_t), DAY_WAVES, REINA_MAX_SCAN_WAVES, REINA_MAX_DAYS,
                          REINA_LDS_ROWS, REINA_LDS_CROWS, OPEN_WEEKLY_IN_STREAM, DAY_SPARSE_MIN_TILES};
    return c[k];
}
}
'''
SHAPE_FIELDS = ('n_agents', 'n_cus', 'n_shards', 'exact', 'hosp_ranges', 'hosp_parallel', 'cand_ovf_cap', 'max_work_items', 'xchg_cap',
                'import_wgs', 'walk_div', 'vacc_one_wg', 'open_tickets', 'imports_in_open', 'day_mode', 'lds_rows_cap', 'small_wgs')
PLAN_FIELDS = ('open_grid', 'open_mode', 'open_tickets', 'weekly_own', 'trace1_in_open', 'xtrace', 'trace1_grid', 'xchg_grid', 'vacc_grid',
               'vacc_parallel', 'vacc_g', 'lds_rows', 'lds_crows', 'day_blocks', 'stream_imports', 'sparse', 'scan_waves', 'scan_tiles',
               'presort_grid', 'remote_grid', 'install_grid', 'install_flags', 'n_walk', 'install_walk_lds')


class LaunchShape(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in SHAPE_FIELDS]


class DayPlan(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32 if n == 'weekly_own' else ctypes.c_uint16 * eng.MAX_VACCINATIONS if n == 'vacc_g' else ctypes.c_uint32)
                for n in PLAN_FIELDS]


_lib = None


def lib():
    """the shim, compiled once a process into a directory of its own"""
    global _lib
    if _lib is None:
        tmp = tempfile.mkdtemp(prefix='reina_launch_')
        src, so = os.path.join(tmp, 'shim.cpp'), os.path.join(tmp, 'libshim.so')
        with open(src, 'w') as f:
            f.write(SHIM % HEADER)
        subprocess.run(['g++', '-O1', '-std=c++17', '-Wall', '-Werror', '-Wno-unused-function', '-fPIC', '-shared', '-o', so, src], check=True)
        _lib = ctypes.CDLL(so)
        for n in ('shim_member_cap', 'shim_lds_rows_for', 'shim_constant'):
            getattr(_lib, n).restype = ctypes.c_uint32
        sizes = [_lib.shim_constant(k) for k in range(3)]
        assert sizes == [ctypes.sizeof(LaunchShape), ctypes.sizeof(DayPlan), ctypes.sizeof(eng.Day)], sizes
    return _lib


def constant(name):
    return lib().shim_constant(3 + ('DAY_WAVES', 'MAX_SCAN_WAVES', 'MAX_DAYS', 'LDS_ROWS', 'LDS_CROWS', 'WEEKLY_IN_STREAM', 'SPARSE_MIN_TILES').index(name))


# ------------------------------------------------------------------------------------------------ the case grid
NO_TESTING, CT, ALL_WITH_SYMPTOMS, ONLY_SEVERE = 0, 1, 2, 3   # reina_prims.h: RT_*
SIZES = (1027, 20000, 8000000, 8000001, 10 ** 8)
GROUPS = (1, 3, 128, 300)   # 300: above n_cus, where every member_cap site is at its floor
N_CUS = 256


def shape(n, n_shards=1, exact=0, **switches):
    """what reina_create derives for a population of n agents made by model.Context (max_work_items = n + 1024, an overflow
    list of (2 x 2^20 - 1024) / 2 records), with the switches' defaults"""
    s = dict(n_agents=n, n_cus=N_CUS, n_shards=n_shards, exact=exact, hosp_ranges=eng.hosp_ranges(n),
             hosp_parallel=int(n > 128 * eng.MAX_HOSP_EVENTS or n_shards > 1), cand_ovf_cap=1048064, max_work_items=n + 1024,
             xchg_cap=16384 if exact else 0, import_wgs=16, walk_div=16, vacc_one_wg=0, open_tickets=0, imports_in_open=0, day_mode=0,
             lds_rows_cap=0, small_wgs=32)
    s.update(switches)
    return s


def day(day=30, testing=ALL_WITH_SYMPTOMS, weekly=0, intervention=0, programmes=()):
    return dict(day=day, testing=testing, weekly=weekly, intervention=intervention, programmes=[list(p) for p in programmes])


def cases():
    """{name: (shape, K, testing_ever, rows, crows, day)}"""
    out = {}

    def add(name, sh, K=1, ever=1, rows=20, crows=16, d=None):
        assert name not in out, name
        out[name] = (sh, K, ever, rows, crows, d or day())

    for n, K in itertools.product(SIZES, GROUPS):
        add('quiet-N%d-K%d' % (n, K), shape(n), K)
        for weekly, iv in itertools.product((1, 512, 513, 9000), (0, 70)):
            add('imports-N%d-K%d-weekly%d-intervention%d' % (n, K, weekly, iv), shape(n), K, d=day(weekly=weekly, intervention=iv))
        add('intervention-only-N%d-K%d' % (n, K), shape(n), K, d=day(intervention=1500))
        for mode, ever in itertools.product((NO_TESTING, CT, ALL_WITH_SYMPTOMS, ONLY_SEVERE), (0, 1)):
            add('testing-N%d-K%d-mode%d-ever%d' % (n, K, mode, ever), shape(n), K, ever, d=day(testing=mode))
        add('last-day-N%d-K%d' % (n, K), shape(n), K, d=day(day=constant('MAX_DAYS') - 1, weekly=600))
        add('tight-overflow-N%d-K%d' % (n, K), shape(n, cand_ovf_cap=1000), K, d=day(weekly=600))   # 2 x 600 records do not fit beside the stream's
        for name, sw in (('import_wgs1', dict(import_wgs=1)), ('walk_div64', dict(walk_div=64)), ('open_tickets', dict(open_tickets=1)),
                         ('imports_in_open', dict(imports_in_open=1)), ('dense', dict(day_mode=1)), ('sparse', dict(day_mode=2)),
                         ('alternate', dict(day_mode=3)), ('lds_rows_cap3', dict(lds_rows_cap=3)), ('small_wgs8', dict(small_wgs=8))):
            add('switch-%s-N%d-K%d' % (name, n, K), shape(n, **sw), K, d=day(weekly=9000))
        add('switch-alternate-odd-N%d-K%d' % (n, K), shape(n, day_mode=3), K, d=day(day=31))
        add('rows-beyond-lds-N%d-K%d' % (n, K), shape(n), K, rows=101, crows=101)
    for n, shards in itertools.product((30000, 8000001), (2, 16)):   # a shard of n agents
        for exact, mode in itertools.product((0, 1), (CT, ALL_WITH_SYMPTOMS)):
            add('shard-N%d-of%d-%s-mode%d' % (n, shards, 'exact' if exact else 'mirror', mode), shape(n, shards, exact), d=day(testing=mode, weekly=20))
    # the vaccination days of tools/launch_trace.py: 200 000 agents, programmes above a step of 16 x 1024 doses a day
    for K in (1, 3, 300):
        add('vacc-chain-K%d' % K, shape(200000), K, d=day(programmes=[(20000, 30000, 200000)]))
        add('vacc-disjoint-K%d' % K, shape(200000), K, d=day(programmes=[(18571, 30000, 100000), (18571, 100000, 200000)]))
        add('vacc-overlapping-K%d' % K, shape(200000), K, d=day(programmes=[(18571, 30000, 130000), (18571, 90000, 200000)]))
        add('vacc-one-wg-K%d' % K, shape(200000, vacc_one_wg=1), K, d=day(programmes=[(20000, 30000, 200000)]))
        add('vacc-small-K%d' % K, shape(200000), K, d=day(programmes=[(1000, 30000, 200000)]))
        add('vacc-window-clips-K%d' % K, shape(200000), K, d=day(programmes=[(10 ** 6, 30000, 40000)]))
        add('vacc-16-tiers-K%d' % K, shape(10 ** 8), K, d=day(programmes=[(400000, k * 10 ** 6, (k + 1) * 10 ** 6) for k in range(16)]))
        add('vacc-few-work-items-K%d' % K, shape(200000, max_work_items=8000), K, d=day(programmes=[(20000, 30000, 200000)]))
    return out


def plan(sh, K, ever, rows, crows, d):
    """(refusal, {field: value}) of one case"""
    cd = eng.Day()
    cd.day, cd.testing_mode = d['day'], d['testing']
    for count, pre_init in ((d['intervention'], 1), (d['weekly'], 0)):
        if count:
            b = cd.import_batches[cd.n_import_batches]
            b.count, b.pre_init = count, pre_init
            cd.n_import_batches += 1
    for k, (nr, first, end) in enumerate(d['programmes']):
        v = cd.vaccinations[k]
        v.nr, v.idx_start, v.idx_end, v.slot = nr, first, end, k
    cd.n_vaccinations = len(d['programmes'])
    p = DayPlan()
    rc = lib().shim_plan_day(ctypes.byref(LaunchShape(**sh)), K, ever, rows, crows, ctypes.byref(cd), ctypes.byref(p))
    return rc, {n: (list(p.vacc_g) if n == 'vacc_g' else int(getattr(p, n))) for n in PLAN_FIELDS}


@pytest.fixture(scope='module')
def plans():
    return {name: (c, plan(*c)) for name, c in cases().items()}


# ------------------------------------------------------------------------------------------------ recorded
def test_the_plans_are_the_recorded_ones(plans):
    with open(RECORD) as f:
        want = json.load(f)
    assert want['fields'] == list(PLAN_FIELDS)
    assert sorted(want['plans']) == sorted(plans)
    for name, (_, (rc, p)) in plans.items():
        assert rc == 0, name
        assert [p[n] for n in PLAN_FIELDS] == want['plans'][name], name


# what the kernel trace of tools/launch_trace.py shows for the cases of the grid it reaches (threads of a grid / 1024):
# {case: {plan field: value}}; read off the trace on one MI355X (256 compute units) before the record was written
TRACED = {
    'quiet-N20000-K1': dict(open_grid=3, day_blocks=3, install_grid=3),
    'quiet-N20000-K3': dict(open_grid=3, day_blocks=3, install_grid=3),
    'quiet-N8000000-K1': dict(open_grid=66, day_blocks=256, sparse=0, install_grid=254),
    'quiet-N8000001-K1': dict(open_grid=66, day_blocks=256, sparse=0, install_grid=254),
    'vacc-chain-K1': dict(vacc_grid=2, open_grid=6, day_blocks=25, install_grid=11), 'vacc-disjoint-K1': dict(vacc_grid=4),
    'vacc-overlapping-K1': dict(vacc_grid=2), 'vacc-one-wg-K1': dict(vacc_grid=1),
}


def test_the_traced_cases_carry_what_the_trace_shows(plans):
    for name, want in TRACED.items():
        p = plans[name][1][1]
        assert {k: p[k] for k in want} == want, name


# ------------------------------------------------------------------------------------------------ asserted from the code's comments
def test_refusals_come_first_and_in_order():
    sh = shape(20000)
    assert plan(sh, 1, 1, 20, 16, day(day=constant('MAX_DAYS')))[0] == 1
    d = eng.Day()
    p = DayPlan()
    for field in ('n_import_batches', 'n_vaccinations'):
        d.day, d.n_import_batches, d.n_vaccinations = 0, 0, 0
        setattr(d, field, 17)
        assert lib().shim_plan_day(ctypes.byref(LaunchShape(**sh)), 1, 1, 20, 16, ctypes.byref(d), ctypes.byref(p)) == 2
        d.day = constant('MAX_DAYS')
        assert lib().shim_plan_day(ctypes.byref(LaunchShape(**sh)), 1, 1, 20, 16, ctypes.byref(d), ctypes.byref(p)) == 1


def test_member_cap_is_a_share_of_the_chip_and_never_nothing():
    for n_cus, K in itertools.product((2, 64, 256, 304), (1, 2, 3, 128, 256, 257, 300, 65535)):
        assert lib().shim_member_cap(n_cus, K) == (n_cus if K == 1 else max(1, n_cus // K))


def test_the_bounds_the_code_promises(plans):
    waves, in_stream = constant('DAY_WAVES'), constant('WEEKLY_IN_STREAM')
    for name, ((sh, K, ever, rows, crows, d), (rc, p)) in plans.items():
        cap = lib().shim_member_cap(sh['n_cus'], K)
        # every later kernel walks scan_waves per-wave slices of lists sized for REINA_MAX_SCAN_WAVES
        assert p['scan_waves'] == p['day_blocks'] * waves <= constant('MAX_SCAN_WAVES') and p['day_blocks'] >= 1, name
        # the streaming workgroups and those that place the imports beside them "all fit the chip together"
        if cap > p['stream_imports']:
            assert p['day_blocks'] + p['stream_imports'] <= cap, name
        assert (p['weekly_own'] == in_stream) == (p['stream_imports'] > 0), name
        # a chained vaccination launch stays resident as a whole
        assert (p['vacc_grid'] > 0) == bool(d['programmes']), name
        if p['vacc_grid'] > 1:
            assert p['vacc_grid'] <= min(256, cap), name
        assert p['vacc_parallel'] == 0 or sum(p['vacc_g']) == p['vacc_grid'], name
        # a single engine's install launch: one workgroup per CU at the most, while the walkers leave two CUs for the installs
        if K == 1 and p['n_walk'] <= sh['n_cus'] - 2:
            assert p['install_grid'] <= sh['n_cus'], name
        assert p['install_grid'] >= (3 if K == 1 else 2) and p['install_walk_lds'] == sh['hosp_parallel'], name
        # the opening: mode 0 until anyone tested, level 1 in a launch of its own only above 8 000 000 agents; tracing level by level under exact attribution
        assert (p['open_mode'] == 0) == (not ever), name
        assert p['trace1_in_open'] == int(ever and d['testing'] == CT and sh['n_agents'] > 8000000 and not sh['exact']), name
        assert p['xtrace'] == int(sh['exact'] and d['testing'] == CT) and (p['xchg_grid'] > 0) == bool(sh['exact']), name
        assert (p['presort_grid'] > 0) == (p['remote_grid'] > 0) == (sh['n_shards'] > 1), name
        assert p['lds_rows'] == lib().shim_lds_rows_for(ctypes.byref(LaunchShape(**sh)), rows, constant('LDS_ROWS')) <= constant('LDS_ROWS'), name
        assert p['lds_crows'] <= constant('LDS_CROWS') and (not sh['lds_rows_cap'] or max(p['lds_rows'], p['lds_crows']) <= sh['lds_rows_cap']), name
        if sh['day_mode'] == 0:
            assert p['sparse'] == int(p['scan_tiles'] >= constant('SPARSE_MIN_TILES') * p['scan_waves']), name


if __name__ == '__main__':
    if '--record' not in sys.argv:
        sys.exit('usage: python tests/test_launch_plan.py --record')
    made = {name: plan(*c) for name, c in cases().items()}
    assert all(rc == 0 for rc, _ in made.values())
    with open(RECORD, 'w') as f:
        f.write('{"fields": %s,\n"plans": {\n%s\n}}\n' % (json.dumps(list(PLAN_FIELDS)), ',\n'.join(
            '%s: %s' % (json.dumps(name), json.dumps([p[n] for n in PLAN_FIELDS])) for name, (_, p) in sorted(made.items()))))
    print('%d plans written to %s' % (len(made), RECORD))
