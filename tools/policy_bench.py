"""Triggered-intervention timings on one GPU.  Writes profiles/policy_bench.json (or --out).  Kernel times come from a separate
run of this script under `rocprofv3 --kernel-trace --stats` (`--quick`; profiles/policy_kernel_stats.csv).

Every leg is the wall time of one whole run on a fresh Context (made and synchronised outside the timed region), the final
wait and read-back included:
  plain        ctx.run(365), no policy -- only API that exists without this feature, so the same script measures a checkout
               of the PARENT commit placed beside the tree (--parent DIR): `parent_plain`
  never        ctx.run(365) with a policy whose thresholds are never met: what carrying a policy costs (one more dependent
               launch a day)
  ward         ctx.run(365) with the people-in-ward policy of the tests (three levels; it switches six times)
  host_driven  the same policy by policy.run_host_driven on the GPU: one blocking round trip a day -- the only way to get the
               behaviour without k_policy
  group128 / host_driven128   128 HUS seeds under the ward policy as ONE policy group, against 128 host-driven runs one after
               the other (--group-days, default 365)
The single-engine legs run alternating (parent_plain, plain, never, ward, host_driven, parent_plain, ...), each in a worker
process of its own that stays alive, a warm-up round first; medians of --reps rounds.
usage: python tools/policy_bench.py [--parent DIR] [--reps N] [--quick] [--out PATH]"""
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
DAYS = 365


def _policies(pol):
    ward = pol.Policy(pol.Signal('in_ward'), levels=[[], [['limit-mobility', 30]], [['limit-mobility', 50], ['wear-masks', 40]]],
                      up=[200, 600], down=[100, 400], review_every=7, min_days=14)
    never = pol.Policy(pol.Signal('dead'), levels=[[], [['limit-mobility', 30]]], up=[2 ** 31 - 1], down=[0])
    return ward, never


def worker(root):
    """one tree's legs on request: a leg name on stdin -> a JSON line on stdout"""
    sys.path.insert(0, root)
    import torch
    from reina_model_amd import simulation
    from reina_model_amd.variables import VARIABLE_DEFAULTS
    try:
        from reina_model_amd import policy as pol
        ward, never = _policies(pol)
    except ImportError:
        pol = ward = never = None
    v = copy.deepcopy(VARIABLE_DEFAULTS)

    def one(leg, days, seed):
        kw = {}
        if leg in ('never', 'ward'):
            kw['policy'] = never if leg == 'never' else ward
        ctx = simulation.make_context(v, seed=seed, ipc='auto', **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if leg == 'host_driven':
            pol.run_host_driven(ctx, ward, days)
        else:
            ctx.run(days)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        lv = getattr(ctx, 'policy_levels', None)
        return dict(ms=ms, switches=int(np.count_nonzero(np.diff(np.concatenate([[0], lv])))) if lv is not None else 0)

    print(json.dumps(dict(ready=True)), flush=True)
    for line in sys.stdin:
        leg, days, seed = line.split()
        print(json.dumps(one(leg, int(days), int(seed))), flush=True)


class Worker:
    def __init__(self, root):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), '--worker', '--root', root], stdin=subprocess.PIPE,
                                  stdout=subprocess.PIPE, text=True, cwd=root)
        assert json.loads(self.p.stdout.readline())['ready']

    def run(self, leg, days, seed=1):
        self.p.stdin.write('%s %d %d\n' % (leg, days, seed))
        self.p.stdin.flush()
        line = self.p.stdout.readline()
        if not line:
            raise RuntimeError('worker died on leg %s' % leg)
        return json.loads(line)

    def close(self):
        self.p.stdin.close()
        self.p.wait(timeout=60)


def spread(ts):
    return dict(median_ms=float(np.median(ts)), min_ms=float(np.min(ts)), max_ms=float(np.max(ts)), all_ms=[float(t) for t in ts])


def single_engine(parent, reps, days):
    legs = [('plain', ROOT), ('never', ROOT), ('ward', ROOT), ('host_driven', ROOT)]
    if parent:
        legs.insert(0, ('parent_plain', parent))
    workers = {name: Worker(root) for name, root in legs}
    try:
        ts = {name: [] for name, _ in legs}
        info = {}
        for rep in range(reps + 1):          # (round 0 warms every worker up)
            for name, _ in legs:
                r = workers[name].run('plain' if name == 'parent_plain' else name, days)
                if rep:
                    ts[name].append(r['ms'])
                info[name] = r['switches']
    finally:
        for w in workers.values():
            w.close()
    out = {name: dict(spread(t), level_changes=info[name]) for name, t in ts.items()}
    med = lambda k: out[k]['median_ms']
    base = 'parent_plain' if parent else 'plain'
    out['ratios'] = dict(never_over_baseline=med('never') / med(base), baseline=base,
                         plain_over_baseline=med('plain') / med(base),
                         never_extra_us_per_day=(med('never') - med(base)) * 1e3 / days,
                         host_driven_over_ward=med('host_driven') / med('ward'), ward_over_baseline=med('ward') / med(base))
    return out


def group(K, days, host_reps):
    sys.path.insert(0, ROOT)
    import torch
    from reina_model_amd import ensemble, policy as pol, simulation
    from reina_model_amd.variables import VARIABLE_DEFAULTS
    ward, _ = _policies(pol)
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    seeds = list(range(1, K + 1))
    ts = []
    for rep in range(2):                      # (the first run warms up; contexts and plan are made outside the timed region)
        ctxs = [simulation.make_context(v, seed=sd, ipc='auto') for sd in seeds]
        plan = simulation.make_context(v, seed=seeds[0], ipc='auto').make_plan(days, policy=ward)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ensemble.run_group_plan(ctxs, plan, policy=ward)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
        levels = [c.policy_levels for c in ctxs]
        distinct = len(set(int(np.argmax(lv > 0)) for lv in levels if lv.any()))
        del ctxs
    # the members one after the other, host-driven (contexts made outside the timed region)
    hd = []
    for sd in seeds[:host_reps]:
        ctx = simulation.make_context(v, seed=sd, ipc='auto')
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pol.run_host_driven(ctx, ward, days)
        torch.cuda.synchronize()
        hd.append((time.perf_counter() - t0) * 1e3)
        del ctx
    hd_total = float(np.sum(hd)) * K / len(hd)
    return dict(K=K, days=days, group_ms=ts[1], group_first_ms=ts[0], distinct_first_escalation_days=distinct,
                host_driven_runs_timed=len(hd), host_driven_ms_per_run=float(np.median(hd)), host_driven_ms_for_K=hd_total,
                host_driven_over_group=hd_total / ts[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--worker', action='store_true')
    ap.add_argument('--root', default=ROOT)
    ap.add_argument('--parent', default=None, help='a built checkout of the parent commit: the baseline leg runs there')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--quick', action='store_true', help='for the rocprofv3 run: one run of the never and the ward policy, a 128-member group of 60 days')
    ap.add_argument('--group-days', type=int, default=DAYS)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'policy_bench.json'))
    a = ap.parse_args()
    if a.worker:
        return worker(a.root)
    sys.path.insert(0, ROOT)
    import torch
    res = dict(device=torch.cuda.get_device_name(0), days=DAYS)
    if a.quick:
        # (in-process, so that the profiler sees the kernels)
        from reina_model_amd import policy as pol, simulation
        from reina_model_amd.variables import VARIABLE_DEFAULTS
        ward, never = _policies(pol)
        for p in (never, ward):
            simulation.make_context(copy.deepcopy(VARIABLE_DEFAULTS), seed=1, ipc='auto', policy=p).run(DAYS)
        res['group'] = group(128, 60, 1)
    else:
        res['single_engine'] = single_engine(a.parent, a.reps, DAYS)
        print(json.dumps(res['single_engine']['ratios']), flush=True)
        res['group'] = group(128, a.group_days, 128)
    print(json.dumps(res['group']), flush=True)
    if a.out and a.out != os.devnull:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
