"""What a logged policy run costs, and the regime report's timings, on one GPU.  Writes profiles/regime_bench.json (or --out).

Scenario: HUS x 365 days under tests/policy_util.py's ward_policy (people in ward, reviewed weekly, three levels).  Every leg
runs in a process of its own (a fresh HIP context, allocator and library each time); the legs alternate, round after round, and
the file keeps the median, min and max of --reps rounds after one warm-up round:
  parent_plain, parent_policy    Context.run without and with the policy on a BUILT checkout of the parent commit (--parent PATH;
                                 without it these legs are left out)
  plain, policy                  the same two on this tree: their medians must lie inside the parent's min-max spread of the same session
                                 (the tool writes the file and then fails when one does not)
  policy_log, policy_course      the policy run with a transmission log, and with the course log too
  report                         one process: the policy + course run once, then ctx.transmission_log.regime_report() as a user calls
                                 it (labels from the run's levels, launch, wait, read-back, the Report object), the log report of the
                                 same state with n_days = 1 (k_txlog_report without its tables by day) and with n_days = 365,
                                 regime.report_numpy on the read-back state, and the read-back; the tool asserts that the device
                                 report equals report_numpy word for word
A leg's time is the wall time of Context.run(365) alone: the history comes back with it (the run's one wait).
usage: python tools/regime_bench.py [--reps N] [--parent PATH] [--out PATH]      (the driver)
       python tools/regime_bench.py --leg NAME [--root PATH]                     (one leg; prints one JSON line)"""
import argparse
import copy
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DAYS = 365
LEGS = ('plain', 'policy', 'policy_log', 'policy_course')
LEG_LIMIT = 300   # seconds a leg's process may take


def spread(ts):
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts), n=len(ts))


def leg(name, root):
    """one leg in this process, on the package under `root`"""
    sys.path[:0] = [root, os.path.join(root, 'tests')]
    from policy_util import ward_policy   # (the tests' policy, not a copy of it)
    from reina_model_amd import simulation
    from reina_model_amd.variables import VARIABLE_DEFAULTS
    kw = {}
    if name != 'plain':
        kw['policy'] = ward_policy()
    if name == 'policy_log':
        kw['txlog'] = True
    if name in ('policy_course', 'report'):
        kw['course'] = True
    ctx = simulation.make_context(copy.deepcopy(VARIABLE_DEFAULTS), seed=1, **kw)
    t0 = time.perf_counter()
    hist = ctx.run(DAYS)
    out = dict(leg=name, run_ms=(time.perf_counter() - t0) * 1e3, agents=int(ctx.engine.config.n_agents), days=int(len(hist)))
    if name != 'plain':
        out['levels_reached'] = sorted(set(int(x) for x in ctx.policy_levels))
    if name == 'report':
        out.update(report_leg(ctx))
    print(json.dumps(out), flush=True)


def timed(fn, reps=9):
    ts = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        res = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return res, dict(spread(ts[1:]), first_ms=ts[0])


def report_leg(ctx):
    import numpy as np
    from reina_model_amd import regime as rgm, reports
    tlog = ctx.transmission_log
    rep, t_rep = timed(tlog.regime_report)
    _, t_log1 = timed(lambda: tlog.report(n_days=1))
    _, t_log = timed(lambda: tlog.report(n_days=DAYS))

    def read_back():
        hot, infector, n_infected, _ = reports.host_state(ctx.engine)
        return hot, infector, n_infected, tlog.words()

    state, t_read = timed(read_back)
    table, labels = ctx._tx_groups(None)[0], rgm.policy_labels(ctx, DAYS)
    spec, t_numpy = timed(lambda: rgm.report_numpy(*state, ctx.age_start, table, labels, DAYS))
    assert np.array_equal(spec.words, rep.words), 'the device report differs from report_numpy of the read-back state'
    rn = rep.reproduction_number()
    return dict(regime_report=t_rep, log_report_n_days_1=t_log1, log_report=t_log, read_back=t_read, numpy=t_numpy,
                scalars={k: int(getattr(rep, k)) for k in rgm.SCALAR_NAMES}, days_by_slot=[int(x) for x in rep.days],
                r_c=[None if x != x else float(x) for x in rn['r_c']], cohort=[int(x) for x in rn['cohort']],
                generation_mean=[rep.generation_interval(r).mean() for r in range(3)],
                presymptomatic_share=[None if x != x else float(x) for x in rep.presymptomatic_share()][:3],
                crossing=[[int(x) for x in row[:3]] for row in rep.crossing[:3]])


def child(name, root):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--leg', name, '--root', root], capture_output=True, text=True, cwd=root,
                       timeout=LEG_LIMIT)
    if r.returncode != 0:
        sys.exit('regime_bench: leg %s under %s failed (%d):\n%s' % (name, root, r.returncode, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--leg')
    ap.add_argument('--root', default=ROOT)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--parent', help='a built checkout of the parent commit: its plain and policy legs join the rounds')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'regime_bench.json'))
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg, os.path.abspath(a.root))
    import torch
    if not torch.cuda.is_available():
        sys.exit('regime_bench: no GPU visible; timings are taken on the device only')
    legs = [(n, ROOT) for n in LEGS]
    if a.parent:
        legs = [('parent_plain', os.path.abspath(a.parent)), ('parent_policy', os.path.abspath(a.parent))] + legs
    times = {n: [] for n, _ in legs}
    facts = {}
    for rnd in range(a.reps + 1):          # (round 0 warms up: page cache, code objects, clocks)
        for n, root in legs:
            r = child(n.replace('parent_', ''), root)
            facts[n] = {k: v for k, v in r.items() if k not in ('run_ms', 'leg')}
            if rnd:
                times[n].append(r['run_ms'])
    res = dict(device=torch.cuda.get_device_name(0), tool='tools/regime_bench.py', days=DAYS, rounds=a.reps,
               legs={n: dict(spread(ts), **facts[n]) for n, ts in times.items()}, report=child('report', ROOT))
    if a.parent:
        L = res['legs']
        res['unlogged_inside_parent_spread'] = {n: bool(L['parent_' + n]['min_ms'] <= L[n]['median_ms'] <= L['parent_' + n]['max_ms'])
                                                for n in ('plain', 'policy')}
    print(json.dumps(res), flush=True)
    if a.out and a.out != os.devnull:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
    outside = [n for n, ok in res.get('unlogged_inside_parent_spread', {}).items() if not ok]
    if outside:
        sys.exit('regime_bench: the unlogged %s leg of this tree lies outside the parent\'s min-max spread' % ' and '.join(outside))


if __name__ == '__main__':
    main()
