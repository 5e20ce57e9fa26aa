"""Dated-transmission-log timings on one GPU.  Writes profiles/txlog_bench.json (or --out).  Kernel times come from a separate
run of this script under `rocprofv3 --kernel-trace --stats` (`--quick`; profiles/txlog_kernel_stats.csv).

Every leg is the wall time of one whole run on a fresh Context (made and synchronised outside the timed region), the final
wait and read-back included:
  plain        ctx.run(days), no log -- the only API that exists without this feature, so the same script measures a built
               checkout of the PARENT commit placed beside the tree (--parent DIR): `parent_plain`
  logged       ctx.run(days) with txlog=True, k_txlog_day in its hot-word form (the default)
  logged_log   the same with REINA_TXLOG_FORM=log: the log word of every active agent is read
The legs run alternating (parent_plain, plain, logged, logged_log, parent_plain, ...), each in a worker process of its own
that stays alive, a warm-up round first; medians of --reps rounds with min and max.  Three sizes: HUS x 365 days, --big agents
(default 1e8) x 130 days (through the first peak), and a 128-member HUS group x 365 days (plain against logged).  The bytes a
day's record launch must move are computed from the shapes and the run's own counters: N / 8 for the bit plane plus one
128-byte line for every agent whose hot word it fetches (the agents infected or not yet counted: the history's `infected`
column is used, a lower bound) -- and as many again for the log words in the `log` form.
A report as a user calls it (launches + read-back) is timed on HUS day 200, the big population's day 120 and the group.
usage: python tools/txlog_bench.py [--parent DIR] [--reps N] [--big N] [--quick] [--out PATH]"""
import argparse
import copy
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DAYS, BIG_DAYS, HBM = 365, 130, 6.3e12


def worker(root):
    """one tree's legs on request: `leg agents days seed` on stdin -> a JSON line on stdout"""
    sys.path.insert(0, root)
    import torch
    from reina_model_amd import datasets, simulation
    from reina_model_amd import engine as eng
    from reina_model_amd.variables import VARIABLE_DEFAULTS
    v = copy.deepcopy(VARIABLE_DEFAULTS)

    def one(leg, agents, days, seed):
        kw = {}
        if leg.startswith('logged') or leg == 'coursed':
            kw['txlog'] = True
            os.environ['REINA_TXLOG_FORM'] = 'log' if leg == 'logged_log' else 'hot'
        if leg == 'coursed':   # (tools/course_bench.py: the clinical course log beside the transmission log)
            kw['course'] = True
        ages = datasets.scaled_population(agents) if agents else None
        ctx = simulation.make_context(v, age_counts=ages, seed=seed, ipc='auto', **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hist = ctx.run(days)
        torch.cuda.synchronize()
        out = dict(ms=(time.perf_counter() - t0) * 1e3, n_agents=int(ctx.total_people))
        ci = eng.C_NAMES.index('infected')
        out['infected_by_day'] = [int(x) for x in np.asarray(hist)[:, ci * eng.MAX_AGES:(ci + 1) * eng.MAX_AGES].sum(axis=1)]
        if leg == 'coursed':
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = ctx.course_log.report()
            out['report_ms'] = (time.perf_counter() - t0) * 1e3
            out['report_infected'], out['with_outcome'], out['with_admission'] = r.infected, r.with_outcome, r.with_admission
        if leg == 'logged':
            report_day = min(days, 200 if not agents else 120)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = ctx.transmission_log.report(n_days=report_day)
            out['report_ms'] = (time.perf_counter() - t0) * 1e3
            out['report_infected'], out['report_links'], out['report_days'] = r.infected, r.links, report_day
        return out

    print(json.dumps(dict(ready=True)), flush=True)
    for line in sys.stdin:
        leg, agents, days, seed = line.split()
        print(json.dumps(one(leg, int(agents), int(days), int(seed))), flush=True)


class Worker:
    def __init__(self, root):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), '--worker', '--root', root], stdin=subprocess.PIPE,
                                  stdout=subprocess.PIPE, text=True, cwd=root)
        assert self._read('start')['ready']

    def _read(self, what):
        """the worker's next JSON line (libraries print lines of their own to stdout while they load)"""
        while True:
            line = self.p.stdout.readline()
            if not line:
                raise RuntimeError('worker died on %s' % what)
            if line.startswith('{'):
                return json.loads(line)

    def run(self, leg, agents, days, seed=1):
        self.p.stdin.write('%s %d %d %d\n' % (leg, agents, days, seed))
        self.p.stdin.flush()
        return self._read('leg %s' % leg)

    def close(self):
        self.p.stdin.close()
        self.p.wait(timeout=60)


def spread(ts):
    return dict(median_ms=float(np.median(ts)), min_ms=float(np.min(ts)), max_ms=float(np.max(ts)), all_ms=[float(t) for t in ts])


def record_bytes(n_agents, infected_by_day, form):
    """bytes k_txlog_day must move on each day (see the module text): (mean, peak day)"""
    per = np.asarray(infected_by_day, dtype=np.float64) * (256.0 if form == 'log' else 128.0) + n_agents / 8.0
    return float(per.mean()), float(per.max())


def single(parent, reps, agents, days):
    legs = [('plain', ROOT), ('logged', ROOT), ('logged_log', ROOT)]
    if parent:
        legs.insert(0, ('parent_plain', parent))
    workers = {name: Worker(root) for name, root in legs}
    try:
        ts = {name: [] for name, _ in legs}
        last = {}
        for rep in range(reps + 1):          # (round 0 warms every worker up)
            for name, _ in legs:
                r = workers[name].run('plain' if name == 'parent_plain' else name, agents, days)
                if rep:
                    ts[name].append(r['ms'])
                last[name] = r
    finally:
        for w in workers.values():
            w.close()
    out = {name: spread(t) for name, t in ts.items()}
    med = lambda k: out[k]['median_ms']
    n = last['plain']['n_agents']
    out['n_agents'], out['days'] = n, days
    base = 'parent_plain' if parent else 'plain'
    out['ratios'] = dict(baseline=base, plain_over_baseline=med('plain') / med(base),
                         plain_inside_baseline_min_max=bool(out[base]['min_ms'] <= med('plain') <= out[base]['max_ms']),
                         logged_over_plain=med('logged') / med('plain'), logged_extra_us_per_day=(med('logged') - med('plain')) * 1e3 / days,
                         logged_log_over_plain=med('logged_log') / med('plain'),
                         logged_log_extra_us_per_day=(med('logged_log') - med('plain')) * 1e3 / days)
    for form, leg in (('hot', 'logged'), ('log', 'logged_log')):
        mean_b, peak_b = record_bytes(n, last[leg]['infected_by_day'], form)
        out[leg]['record_bytes_mean_day'], out[leg]['record_bytes_peak_day'] = mean_b, peak_b
        out[leg]['record_us_at_hbm_rate_mean_day'], out[leg]['record_us_at_hbm_rate_peak_day'] = mean_b / HBM * 1e6, peak_b / HBM * 1e6
    r = last['logged']
    # a report's least bytes: hot + log of every agent, the cold record (a 32-byte sector) of every infected one, hot + log lines of every link's infector
    least = 8.0 * n + 32.0 * r['report_infected'] + 2 * 128.0 * r['report_links']
    out['report'] = dict(day=r['report_days'], call_ms=r['report_ms'], infected=r['report_infected'], links=r['report_links'],
                         least_bytes=least, fraction_of_hbm_rate=least / HBM / (r['report_ms'] * 1e-3))
    return out


def group(K, days):
    sys.path.insert(0, ROOT)
    import torch
    from reina_model_amd import ensemble, simulation
    from reina_model_amd.variables import VARIABLE_DEFAULTS
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    seeds = list(range(1, K + 1))
    plan = simulation.make_context(v, seed=seeds[0], ipc='auto').make_plan(days)
    ts = {'plain': [], 'logged': []}
    rep_ms = None
    for rep in range(2):                      # (the first round warms up; contexts and plan are made outside the timed region)
        for leg in ('plain', 'logged'):
            ctxs = [simulation.make_context(v, seed=sd, ipc='auto') for sd in seeds]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ensemble.run_group_plan(ctxs, plan, txlog=leg == 'logged')
            torch.cuda.synchronize()
            ts[leg].append((time.perf_counter() - t0) * 1e3)
            if leg == 'logged':
                t0 = time.perf_counter()
                reps = ensemble.log_reports(ctxs)
                rep_ms = (time.perf_counter() - t0) * 1e3
                infected, links = sum(r.infected for r in reps), sum(r.links for r in reps)
                n = ctxs[0].total_people
            del ctxs
    least = 8.0 * n * K + 32.0 * infected + 256.0 * links
    return dict(K=K, days=days, plain_ms=ts['plain'][1], logged_ms=ts['logged'][1], first_round_ms=[ts['plain'][0], ts['logged'][0]],
                logged_over_plain=ts['logged'][1] / ts['plain'][1], logged_extra_us_per_day=(ts['logged'][1] - ts['plain'][1]) * 1e3 / days,
                report=dict(call_ms=rep_ms, infected=infected, links=links, least_bytes=least, fraction_of_hbm_rate=least / HBM / (rep_ms * 1e-3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--worker', action='store_true')
    ap.add_argument('--root', default=ROOT)
    ap.add_argument('--parent', default=None, help='a built checkout of the parent commit: the baseline leg runs there')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--big', type=int, default=10 ** 8)
    ap.add_argument('--big-reps', type=int, default=3)
    ap.add_argument('--group', type=int, default=128)
    ap.add_argument('--quick', action='store_true', help='for the rocprofv3 run: one logged run of each form at HUS and at --big agents, one report each')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'txlog_bench.json'))
    a = ap.parse_args()
    if a.worker:
        return worker(a.root)
    sys.path.insert(0, ROOT)
    import torch
    res = dict(device=torch.cuda.get_device_name(0))
    if a.quick:
        # (in-process, so that the profiler sees the kernels)
        from reina_model_amd import datasets, simulation
        from reina_model_amd.variables import VARIABLE_DEFAULTS
        for agents, days in ((0, DAYS), (a.big, BIG_DAYS)):
            for form in ('hot', 'log'):
                os.environ['REINA_TXLOG_FORM'] = form
                ctx = simulation.make_context(copy.deepcopy(VARIABLE_DEFAULTS), age_counts=datasets.scaled_population(agents) if agents else None,
                                              seed=1, ipc='auto', txlog=True)
                ctx.run(days)
                ctx.transmission_log.report()
                del ctx
        return
    res['hus'] = single(a.parent, a.reps, 0, DAYS)
    print(json.dumps(res['hus']['ratios']), flush=True)
    if a.big:
        res['big'] = single(None, a.big_reps, a.big, BIG_DAYS)
        print(json.dumps(res['big']['ratios']), flush=True)
    if a.group:
        res['group'] = group(a.group, DAYS)
        print(json.dumps(res['group']), flush=True)
    if a.out and a.out != os.devnull:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
