"""Lineage-report timings on one GPU, as a user calls the report.  Writes profiles/lineage_bench.json (or --out).

Two states, each made by a logged run in this process: HUS x 200 days and 10^7 agents x 60 days.  On each, alternating in the
same process after one warm-up call of each:

  lineage    ctx.transmission_log.lineage_report(period=7): five kinds of launch (k_lineage_links, 13 x k_tx_jump,
             k_lineage_tally, k_lineage_roots, k_lineage_finish), one read-back of the report block
  both       ctx.transmission_report() + ctx.transmission_log.report(): the tree report and the log report of the same state --
             code this report leaves untouched, and roughly the work it does (the links are classified twice there, once here)

Every call ends in a read-back of its block, so the host clock around it (after a device synchronise) covers the kernels, the
scratch and report allocations and the copy.  A call is a few milliseconds: the figures are medians of --reps calls with their
spread, and the sum over the calls is given beside them.  A measurement path that finds no GPU fails.

usage: python tools/lineage_bench.py [--reps N] [--big N] [--quick] [--out PATH]"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)


def spread(ts):
    return dict(median_ms=float(np.median(ts)), min_ms=float(np.min(ts)), max_ms=float(np.max(ts)), sum_ms=float(np.sum(ts)),
                all_ms=[round(float(t), 4) for t in ts])


def case(name, agents, days, reps):
    import torch
    from reina_model_amd import datasets, lineage, simulation
    from reina_model_amd.variables import VARIABLE_DEFAULTS
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    ages = datasets.scaled_population(agents) if agents else None
    ctx = simulation.make_context(v, age_counts=ages, seed=5, ipc='auto', txlog=True)
    ctx.run(days, record_history=False)
    log = ctx.transmission_log
    assert log.on_device and ctx.engine.lineage_f is not None

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    legs = dict(lineage=lambda: log.lineage_report(period=7), both=lambda: (ctx.transmission_report(), log.report()))
    ts = {k: [] for k in legs}
    last = {}
    for rep in range(reps + 1):              # (round 0 warms both up)
        for k, f in legs.items():
            ms, last[k] = timed(f)
            if rep:
                ts[k].append(ms)
    r = last['lineage']
    tree, lrep = last['both']
    assert r.infected == tree.n_infected_agents == lrep.infected and r.links == tree.n_linked and r.largest_tree == tree.largest_cluster
    out = dict(case=name, n_agents=int(ctx.total_people), days=days, reps=reps, period_days=r.period_days, n_periods=r.n_periods,
               infected=r.infected, links=r.links, trees=r.trees, alive_trees=r.alive_trees, largest_tree=r.largest_tree,
               rounds=r.rounds, report_bytes=int(lineage.report_words(r.n_periods) * 8),
               lineage=spread(ts['lineage']), both=spread(ts['both']))
    out['lineage_over_both'] = out['lineage']['median_ms'] / out['both']['median_ms']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--big', type=int, default=10 ** 7)
    ap.add_argument('--quick', action='store_true', help='HUS x 60 days and 10^6 agents x 30 days, 3 calls each')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lineage_bench.json'))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('lineage_bench: no GPU visible; timings are taken on the device only')
    cases = [('hus_60d', 0, 60), ('1e6_30d', 10 ** 6, 30)] if a.quick else [('hus_200d', 0, 200), ('%d_60d' % a.big, a.big, 60)]
    reps = 3 if a.quick else a.reps
    out = dict(device=torch.cuda.get_device_name(0), tool='tools/lineage_bench.py', cases=[case(n, ag, d, reps) for n, ag, d in cases])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(out, fh, indent=1)
    for c in out['cases']:
        print('%-14s lineage %.2f ms (%.2f .. %.2f)   tree + log report %.2f ms (%.2f .. %.2f)   ratio %.2f' % (
            c['case'], c['lineage']['median_ms'], c['lineage']['min_ms'], c['lineage']['max_ms'], c['both']['median_ms'],
            c['both']['min_ms'], c['both']['max_ms'], c['lineage_over_both']))


if __name__ == '__main__':
    main()
