"""Clinical-course-log timings on one GPU.  Writes profiles/course_bench.json (or --out).  Kernel times come from a separate
run of this script under `rocprofv3 --kernel-trace --stats` (`--quick`; profiles/course_kernel_stats.csv).

The legs and the way they are timed are tools/txlog_bench.py's (its workers run them): the wall time of one whole run on a
fresh Context, the final wait and read-back included --
  plain        ctx.run(days), no log         (also on a built checkout of the PARENT commit, --parent DIR: `parent_plain`)
  logged       ctx.run(days) with txlog=True (also on the parent: `parent_logged`)
  coursed      ctx.run(days) with course=True: k_course_day in k_txlog_day's place, still one record launch a day
alternating (parent_plain, parent_logged, plain, logged, coursed, parent_plain, ...), each in a worker process of its own that
stays alive, a warm-up round first; medians of --reps rounds with min and max.  Two sizes: HUS x 365 days and --big agents
(default 1e8) x 130 days.  The course report as a user calls it (launch + read-back) is timed at the end of the coursed run.
usage: python tools/course_bench.py [--parent DIR] [--reps N] [--big N] [--quick] [--out PATH]"""
import argparse
import copy
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import txlog_bench as tb  # noqa: E402


def single(parent, reps, agents, days):
    legs = [('plain', ROOT), ('logged', ROOT), ('coursed', ROOT)]
    if parent:
        legs = [('parent_plain', parent), ('parent_logged', parent)] + legs
    workers = {name: tb.Worker(root) for name, root in legs}
    try:
        ts = {name: [] for name, _ in legs}
        last = {}
        for rep in range(reps + 1):          # (round 0 warms every worker up)
            for name, _ in legs:
                r = workers[name].run(name.replace('parent_', ''), agents, days)
                if rep:
                    ts[name].append(r['ms'])
                last[name] = r
    finally:
        for w in workers.values():
            w.close()
    out = {name: tb.spread(t) for name, t in ts.items()}
    med = lambda k: out[k]['median_ms']
    out['n_agents'], out['days'] = last['plain']['n_agents'], days
    out['ms_per_day'] = {name: med(name) / days for name, _ in legs}
    out['ratios'] = dict(coursed_over_logged=med('coursed') / med('logged'), coursed_extra_us_per_day=(med('coursed') - med('logged')) * 1e3 / days,
                         logged_over_plain=med('logged') / med('plain'))
    if parent:
        out['ratios'].update(plain_over_parent=med('plain') / med('parent_plain'), logged_over_parent=med('logged') / med('parent_logged'),
                             plain_inside_parent_min_max=bool(out['parent_plain']['min_ms'] <= med('plain') <= out['parent_plain']['max_ms']),
                             logged_inside_parent_min_max=bool(out['parent_logged']['min_ms'] <= med('logged') <= out['parent_logged']['max_ms']))
    r = last['coursed']
    # a report's least bytes: the hot word of every agent, log word and record of the tiles that hold an infected one (all of them here)
    least = 16.0 * out['n_agents']
    out['report'] = dict(call_ms=r['report_ms'], infected=r['report_infected'], with_outcome=r['with_outcome'], with_admission=r['with_admission'],
                         least_bytes=least, fraction_of_hbm_rate=least / tb.HBM / (r['report_ms'] * 1e-3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default=None, help='a built checkout of the parent commit: the baseline legs run there')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--big', type=int, default=10 ** 8)
    ap.add_argument('--big-reps', type=int, default=3)
    ap.add_argument('--quick', action='store_true', help='for the rocprofv3 run: one coursed and one logged run at HUS (and at --big agents), one report')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'course_bench.json'))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        sys.exit('course_bench: no GPU visible; timings are taken on the device only')
    res = dict(device=torch.cuda.get_device_name(0), tool='tools/course_bench.py')
    if a.quick:
        # (in-process, so that the profiler sees the kernels)
        from reina_model_amd import datasets, simulation
        from reina_model_amd.variables import VARIABLE_DEFAULTS
        for agents, days in ((0, tb.DAYS),) + (((a.big, tb.BIG_DAYS),) if a.big else ()):
            for course in (False, True):
                ctx = simulation.make_context(copy.deepcopy(VARIABLE_DEFAULTS), age_counts=datasets.scaled_population(agents) if agents else None,
                                              seed=1, ipc='auto', txlog=True, course=course)
                ctx.run(days)
                if course:
                    ctx.course_log.report()
                del ctx
        return
    res['hus'] = single(os.path.abspath(a.parent) if a.parent else None, a.reps, 0, tb.DAYS)   # (a worker runs in its tree's directory)
    print(json.dumps(dict(res['hus']['ratios'], ms_per_day=res['hus']['ms_per_day'])), flush=True)
    if a.big:
        res['big'] = single(None, a.big_reps, a.big, tb.BIG_DAYS)
        print(json.dumps(dict(res['big']['ratios'], ms_per_day=res['big']['ms_per_day'])), flush=True)
    if a.out and a.out != os.devnull:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
