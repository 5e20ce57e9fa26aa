"""Ensemble-summary timings on one GPU.  Writes profiles/summary_bench.json (or --out).  Kernel times come from a separate run
of this script under `rocprofv3 --kernel-trace --stats` (profiles/summary_kernel_stats.csv; --quick is made for it).

Workloads: K x HUS x 365 days for K = 128 and K = 64, as a user calls them.  Three routes, in the same process and alternating,
each on fresh members of the same seeds (made outside the clock), after one warm-up ensemble:
  device   ensemble.run_group_plan(members, plan, summary=spec): the kernels, the block read back
  host     ensemble.run_group_plan(members, plan) followed by summary.summarise_numpy on the returned history: what the commit
           before the summary could do
  run      ensemble.run_group_plan(members, plan) alone: the run with its read-back, so the read-back's share is visible
Host clock around a call that ends with its result on the host; median, minimum and maximum of --reps calls.  The summary call
alone is timed as well, on a history that is on the device already: launches to the read-back of the block.
usage: python tools/summary_bench.py [--quick] [--reps N] [--out PATH]"""
import argparse
import copy
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from reina_model_amd import datasets, engine as eng, ensemble, simulation, summary as sm  # noqa: E402
from reina_model_amd.variables import VARIABLE_DEFAULTS  # noqa: E402


def stats(ts):
    return dict(median_ms=float(np.median(ts)), min_ms=float(np.min(ts)), max_ms=float(np.max(ts)), all_ms=[float(t) for t in ts])


def workload(K, days, reps, spec, v, ages):
    import torch
    mk = lambda sd: simulation.make_context(v, age_counts=ages, seed=sd)
    planner = mk(0)
    plan = planner.make_plan(days)

    def members():
        t0 = time.perf_counter()
        m = [mk(100 + k) for k in range(K)]
        torch.cuda.synchronize()
        return m, (time.perf_counter() - t0) * 1e3

    def device(m):
        return ensemble.run_group_plan(m, plan, summary=spec)

    def host(m):
        return sm.summarise_numpy(ensemble.run_group_plan(m, plan), planner.nr_ages, spec, ctx=planner)

    def run(m):
        return ensemble.run_group_plan(m, plan)

    routes = dict(device=device, host=host, run=run)
    warm, make_ms = members()
    ref = device(warm)
    del warm
    times = {name: [] for name in routes}
    for r in range(reps):
        for name, fn in routes.items():
            m, _ = members()
            gc.collect()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(m)
            times[name].append((time.perf_counter() - t0) * 1e3)
            if name == 'device':
                assert out == ref, 'two device summaries of the same seeds differ'
            elif name == 'host':
                assert np.array_equal(out, ref.words), 'the host route and the device route differ'
            del m, out
        print('K=%d rep %d: ' % (K, r) + ', '.join('%s %.1f ms' % (n, times[n][-1]) for n in routes), flush=True)
    # the summary alone, on rows that are on the device: launches to the read-back of the block
    m, _ = members()
    group = eng.EngineGroup([c.engine for c in m])
    try:
        from reina_model_amd.dayrun import History, replay_plan
        hist = History(days, group=group)
        replay_plan(plan, group, hist, lambda si, tables: group.upload_contact_tables(*tables) if tables is not None else None)
        torch.cuda.synchronize()
        rows = hist.rows()
        alone = []
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            s = sm.summarise(rows, planner.nr_ages, spec, ctx=planner)
            alone.append((time.perf_counter() - t0) * 1e3)
        assert s == ref
    finally:
        group.close()
    lay = ref.layout
    return dict(K=K, days=days, agents=planner.engine.config.n_agents, series=lay.S, groups=lay.G, quantiles=lay.Q, thresholds=lay.T,
                history_bytes=K * days * eng.COUNTER_WORDS * 4, report_bytes=lay.words * 8,
                scratch_bytes=sm.scratch_bytes(K, days, lay.S), make_members_ms=make_ms,
                device_route=stats(times['device']), host_route=stats(times['host']), run_alone=stats(times['run']),
                summary_alone=stats(alone[1:]),
                host_over_device=float(np.median(times['host']) / np.median(times['device'])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--quick', action='store_true', help='K = 128 only, 2 calls a route (for the rocprofv3 run)')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--days', type=int, default=365)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'summary_bench.json'))
    a = ap.parse_args()
    import torch
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    ages = datasets.get_population_for_area()
    spec = sm.SummarySpec(thresholds=[('in_icu', v['icu_units']), ('in_ward', v['hospital_beds'])])
    res = dict(device=torch.cuda.get_device_name(0), method='host clock around each call, result on the host; %d calls a route, '
               'alternating, fresh members each call (made outside the clock), after a warm-up ensemble' % (2 if a.quick else a.reps),
               workloads=[])
    for K in (128,) if a.quick else (128, 64):
        res['workloads'].append(workload(K, a.days, 2 if a.quick else a.reps, spec, v, ages))
        print(json.dumps({k: x for k, x in res['workloads'][-1].items()}), flush=True)
        if not a.quick or a.out != ap.get_default('out'):
            with open(a.out, 'w') as f:
                json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
