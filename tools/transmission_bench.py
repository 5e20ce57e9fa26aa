"""Transmission-report timings on one GPU: HUS at day 200, 1e8 agents at day 120, a 128-member HUS engine group, and a synthetic
single cluster.  Writes profiles/transmission_bench.json (or --out).  Kernel times come from a separate run of this script under
`rocprofv3 --kernel-trace --stats` (profiles/transmission_kernel_stats.csv).

Per case: the wall time of one report as a user calls it (launches + the 78 KB read-back, after warmup; median of --reps), and
the least bytes the passes move, from the shapes: links 4 B hot + 8 B pair + 4 B size per agent, 32 B (one sector) per infected
agent's cold record and 4 B per linked agent's infector word; each jump round 16 B per agent (+ 8 B per gathered parent, not
counted); tally 12 B per agent; clusters 4 B per agent.  The fraction is of 6.3 TB/s.
usage: python tools/transmission_bench.py [--quick] [--out PATH]"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from reina_model_amd import datasets, ensemble, simulation, transmission as tx  # noqa: E402
from reina_model_amd.variables import VARIABLE_DEFAULTS  # noqa: E402

PEAK = 6.3e12


def min_bytes(n, r):
    return n * (4 + 8 + 4) + 32 * r.n_infected_agents + 4 * r.n_linked + r.rounds * n * 16 + n * 12 + n * 4


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, float(np.median(ts)), ts


def case_context(name, ages, days, seed, reps):
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    ctx = simulation.make_context(v, age_counts=ages, seed=seed)
    ctx.run(days, record_history=False)
    r, ms, ts = timed(ctx.transmission_report, reps)
    n = ctx.total_people
    b = min_bytes(n, r)
    print('%-22s n=%d day=%d: %.3f ms  %.2f GB  %.1f%% of peak' % (name, n, days, ms, b / 1e9, 100 * b / (ms * 1e-3) / PEAK), flush=True)
    return dict(case=name, n_agents=n, day=days, ms_median=ms, ms_all=ts, min_bytes=b, fraction_of_peak=b / (ms * 1e-3) / PEAK,
                rounds=r.rounds, n_infected_agents=r.n_infected_agents, n_roots=r.n_roots, max_generation=r.max_generation,
                largest_cluster=r.largest_cluster, mean_offspring=r.mean_offspring(), dispersion_k=r.dispersion_k(),
                top20_share=r.top_share(0.2))


def case_group(k, days, reps):
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    ages = datasets.get_population_for_area('HUS')
    ctxs = [simulation.make_context(v, age_counts=ages, seed=s) for s in range(k)]
    ensemble.run_group_plan(ctxs, ctxs[0].make_plan(days), record_history=False)
    from reina_model_amd import engine as eng
    group = eng.EngineGroup([c.engine for c in ctxs])
    reps_, ms, ts = timed(lambda: ensemble.transmission_reports(ctxs, group=group), reps)
    group.close()
    n = ctxs[0].total_people
    b = sum(min_bytes(n, r) for r in reps_)
    print('%-22s K=%d n=%d day=%d: %.3f ms  %.2f GB  %.1f%% of peak' % ('hus_group', k, n, days, ms, b / 1e9, 100 * b / (ms * 1e-3) / PEAK), flush=True)
    return dict(case='hus_group_%d' % k, members=k, n_agents=n, day=days, ms_median=ms, ms_all=ts, min_bytes=b,
                fraction_of_peak=b / (ms * 1e-3) / PEAK, ms_per_member=ms / k)


def case_cluster(n, reps):
    import snap_util
    import tx_util
    hot, inf, cnt = tx_util.forest(n, 'giant')
    ctx = snap_util.make_context(n)
    tx_util.put_forest(ctx, hot, inf, cnt, day=4095)
    g = tx_util.groups()
    r, ms, ts = timed(lambda: tx.report_engine(ctx.engine, g), reps)
    b = min_bytes(n, r)
    print('%-22s n=%d: %.3f ms  %.2f GB  %.1f%% of peak' % ('single_cluster', n, ms, b / 1e9, 100 * b / (ms * 1e-3) / PEAK), flush=True)
    return dict(case='single_cluster', n_agents=n, ms_median=ms, ms_all=ts, min_bytes=b, fraction_of_peak=b / (ms * 1e-3) / PEAK,
                rounds=r.rounds, max_generation=r.max_generation, largest_cluster=r.largest_cluster)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--quick', action='store_true', help='small sizes (the profiler run)')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'transmission_bench.json'))
    a = ap.parse_args()
    big = 10_000_000 if a.quick else 100_000_000
    out = [case_context('hus', datasets.get_population_for_area('HUS'), 200, 5, a.reps),
           case_context('scaled', datasets.scaled_population(big), 120, 2, a.reps)]
    out.append(case_group(16 if a.quick else 128, 200, a.reps))
    out.append(case_cluster(3_000_000 if a.quick else 20_000_000, a.reps))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(dict(peak_bytes_per_s=PEAK, quick=a.quick, cases=out), fh, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
