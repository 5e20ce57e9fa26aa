"""The launches of a fixed list of short runs, observed from outside: which kernels of the library are dispatched, in which
order, with which grid, workgroup size and LDS size.  Results do not depend on launch geometry, so no test of results sees a
wrong grid; this does.  A change to the host code that is meant to leave the launches alone is checked by running the cases
under the kernel trace on the tree before it and on the tree after it and comparing the two traces:

    rocprofv3 --kernel-trace --output-format csv -d OUT -o NAME -- python tools/launch_trace.py
    python tools/launch_trace.py --compare BEFORE_kernel_trace.csv AFTER_kernel_trace.csv

(no counters, no other tracing; `--list` prints the cases without running them).  The environment switches are read in
reina_create, so they are set before each case's make_context and taken back behind it."""
import collections
import copy
import csv
import os
import re
import sys
from datetime import date, timedelta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SMOKE_AGENTS = 20000
VACC_AGENTS = 200000
# the population sizes on both sides of every size threshold of reina_launch.h: REINA_HOSP_SMALL_AGENTS (128 x 16384: the
# bucket-per-wave event walk above it), 8 000 000 (k_open's roles by block number and level-1 tracing in a launch of its own
# above it), and the sparse stream from DAY_SPARSE_MIN_TILES x day_blocks x DAY_WAVES = 4 x 256 x 16 = 16384 tiles of 512
# agents on (8 388 100 agents are the first with 16384 tiles: ((N >> 2) + 127) / 128)
THRESHOLD_SIZES = (2097152, 2097153, 8000000, 8000001, 8388096, 8388100)


def _variables():
    from reina_model_amd.variables import VARIABLE_DEFAULTS
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    v.update(hospital_beds=12, icu_units=2)
    return v


def _ages(n):
    """the HUS age shape with EXACTLY n agents"""
    from reina_model_amd import datasets
    ages = datasets.scaled_population(n)
    ages[40] += n - int(ages.sum())
    return ages


def _day(v, day):
    return (date.fromisoformat(v['start_date']) + timedelta(days=day)).isoformat()


def _single(n, days, programmes=(), **kw):
    from reina_model_amd import simulation
    v = _variables()
    v['interventions'] = list(v['interventions']) + [['vaccinate', _day(v, 5), weekly, lo, hi] for weekly, lo, hi in programmes]
    simulation.make_context(v, age_counts=_ages(n), seed=3, **kw).run(days)


def _group(members, policy=None):
    from reina_model_amd import ensemble
    seeds = list(range(100, 100 + members))
    if policy is None:
        ensemble.run_ensemble(_variables(), seeds, 40, age_counts=_ages(SMOKE_AGENTS))
    else:
        ensemble.run_policy_ensemble(_variables(), seeds, 40, policy, age_counts=_ages(SMOKE_AGENTS))


def _rows_policy():
    """levels whose tables hold different numbers of distinct rows (policy_lds_rows: the most of any level)"""
    from reina_model_amd import policy as pol
    return pol.Policy(pol.Signal('all_infected'), levels=[[], [['limit-mobility', 35, 23, 67]], [['limit-mobility', 55, None, None, 'leisure']]],
                      up=[30, 200], down=[10, 100], review_every=1, min_days=3)


def _shards(attribution):
    """two in-process shards, 20 days of a scenario with contact tracing from day 12 and weekly imports"""
    from reina_model_amd import sharding, simulation
    v = _variables()
    v.update(hospital_beds=30, icu_units=4)
    ivs = [['import-infections', _day(v, 0), 60], ['test-with-contact-tracing', _day(v, 12), 80], ['import-infections-weekly', _day(v, 14), 20, 30]]
    members = []
    cs = [simulation.make_context(v, age_counts=_ages(30000), seed=11, interventions=ivs,
                                  comm=sharding.InProcessComm(r, 2, members, attribution=attribution)) for r in range(2)]
    for _ in range(20):
        sharding.step_shards_together(cs)


def cases():
    """[(name, environment, function)]"""
    out = [('smoke', {}, lambda: _single(SMOKE_AGENTS, 40))]
    for env in ({'REINA_IMPORT_WGS': '1'}, {'REINA_OPEN_TICKETS': '1'}, {'REINA_IMPORTS_IN_OPEN': '1'}, {'REINA_DAY_MODE': 'alternate'},
                {'REINA_LDS_ROWS_CAP': '3'}, {'REINA_FUSED_DAY': '1'}):
        out.append(('smoke-%s' % '-'.join('%s=%s' % kv for kv in env.items()), env, lambda: _single(SMOKE_AGENTS, 40)))
    # (weekly doses: 140 000 are 20 000 a day, above a step of 16 x 1024 agents; every window holds more agents than that)
    out += [('vacc-chain', {}, lambda: _single(VACC_AGENTS, 15, [(140000, 16, 100)])),
            ('vacc-disjoint', {}, lambda: _single(VACC_AGENTS, 15, [(130000, 16, 44), (130000, 45, 100)])),
            ('vacc-overlapping', {}, lambda: _single(VACC_AGENTS, 15, [(130000, 16, 60), (130000, 40, 100)])),
            ('vacc-one-wg', {'REINA_VACC_ONE_WG': '1'}, lambda: _single(VACC_AGENTS, 15, [(140000, 16, 100)]))]
    out += [('group-%d' % k, {}, lambda k=k: _group(k)) for k in (1, 3, 4)]
    out += [('group-policy', {}, lambda: _group(3, _rows_policy())),
            ('logged', {}, lambda: _single(SMOKE_AGENTS, 40, txlog=True)),
            ('shards-exact', {}, lambda: _shards('exact')), ('shards-mirror', {}, lambda: _shards('mirror'))]
    out += [('size-%d' % n, {}, lambda n=n: _single(n, 10)) for n in THRESHOLD_SIZES]
    return out


def run_cases(only=None):
    import torch
    for name, env, fn in cases():
        if only and name not in only:
            continue
        saved = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            fn()
            torch.cuda.synchronize()
        finally:
            for k, x in saved.items():
                if x is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = x
        print('case %s done' % name, flush=True)


def dispatches(path):
    """(library dispatches in order as (kernel, grid, workgroup, LDS bytes), counts of all other kernels)"""
    with open(path, newline='') as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r.get('Dispatch_Id') or r['Start_Timestamp']))
    ours, others = [], collections.Counter()
    for r in rows:
        m = re.search(r'\bk_[a-z0-9_]+(<[^>]*>)?', r['Kernel_Name'])
        if m is None:
            others[r['Kernel_Name'].split('(')[0]] += 1
            continue
        xyz = lambda stem: tuple(int(r['%s_%s' % (stem, a)]) for a in 'XYZ')
        ours.append((m.group(0).replace(' ', ''), xyz('Grid_Size'), xyz('Workgroup_Size'), int(r['LDS_Block_Size'])))
    return ours, others


def compare(path_a, path_b):
    a, others_a = dispatches(path_a)
    b, others_b = dispatches(path_b)
    print('library dispatches: %d | %d' % (len(a), len(b)))
    by_kernel_a, by_kernel_b = collections.Counter(d[0] for d in a), collections.Counter(d[0] for d in b)
    for k in sorted(set(by_kernel_a) | set(by_kernel_b)):
        shapes = len(set(d[1:] for d in a if d[0] == k))
        print('  %-44s %7d | %7d   (%d distinct shapes)' % (k, by_kernel_a[k], by_kernel_b[k], shapes))
    print('other kernels (not compared): %d | %d' % (sum(others_a.values()), sum(others_b.values())))
    for k in sorted(set(others_a) | set(others_b)):
        print('  %-100s %7d | %7d' % (k[:100], others_a[k], others_b[k]))
    first = next((k for k, (x, y) in enumerate(zip(a, b)) if x != y), None)
    if first is None and len(a) == len(b):
        print('IDENTICAL: the two dispatch sequences agree in kernel, grid, workgroup size and LDS size, in order')
        return 0
    first = min(len(a), len(b)) if first is None else first
    print('DIFFERENT from dispatch %d on:' % first)
    for k in range(max(0, first - 3), first + 4):
        print('  %6d  %-90s | %s' % (k, a[k] if k < len(a) else '-', b[k] if k < len(b) else '-'))
    return 1


if __name__ == '__main__':
    if '--compare' in sys.argv:
        at = sys.argv.index('--compare')
        sys.exit(compare(sys.argv[at + 1], sys.argv[at + 2]))
    if '--list' in sys.argv:
        for name, env, _ in cases():
            print(name, env)
        sys.exit(0)
    run_cases(set(sys.argv[1:]) or None)
