"""Particle-filter timings on one GPU.  Writes profiles/filter_bench.json (or --out).  Kernel times come from a separate run
of this script under `rocprofv3 --kernel-trace --stats` (profiles/filter_kernel_stats.csv).

Cases:
  hus_k128   the HUS case file (all_detected and in_ward, r = 10) filtered with K = 128 in 7-day windows over its span from the
             scenario's start date.  Per window: `run` = make_plan + the days + the history read-back (run_group_plan), `score`,
             `resample`, `clone` (host issue of the one launch); the read-back alone is timed on a history block of the same
             shape, and `days` = run - read-back.  Then, after 7 more days of the group as it ends, the clone of the last
             resample's pair list against the snapshot route (pack every distinct source, one unpack per destination), both
             synchronised.
  clone_1e7  K = 16 members of 10^7 agents run 120 days as a group; members 8..15 get the states of members 0..7: the clone
             against the snapshot route on that pair list.
  --params   (alone; writes profiles/params_bench.json) the HUS case without parameters and with one and four knobs
             (filtering.particle_filter(..., parameters=...): reina_params.h), by --logged's protocol: every leg in a process
             of its own, alternating over --rounds rounds, --parent DIR for the parent commit's unlogged leg.  Per leg the
             filter's wall time per window; of the legs with parameters also `params_ms_per_resample` (the Liu-West step, the
             K blocks' expansion on the host for the Contexts and the set's issue) and `params_set_ms`, the synchronised
             reina_group_params_set of all 128 members, median of --reps.
  --logged   (alone; writes profiles/filter_log_bench.json) the HUS case three ways -- unlogged, with the transmission log
             (txlog=True), with log and course (course=True): the filter's wall time per window (synchronised at the end), and,
             after 7 more days, the synchronised clone of the last resample's pair list (reina_group_clone, or
             reina_group_txlog_clone: the log's launch ahead of the state's), median of --reps.  Every leg runs in a process of
             its own, the legs alternating over --rounds rounds (medians, min and max over the rounds); --parent DIR, a built
             checkout of the parent commit, runs the unlogged leg there as well.  --windows W caps the filter at W windows.
             `wall_ms_per_window`: what the windows took (run, score, resample, clone issue; the members' construction is not
             in it) over their number.  Bytes the log's launch adds, from the shapes: 8 B per agent and pair (both hot words),
             and per agent recorded in either member 4 B read + 4 B written of log, 12 + 12 with a course (a dense copy: 8 or
             24 B per agent).
Bytes of a clone, from the shapes and the recorded-agent counts: per pair 8 B per agent (both hot words), 64 B read + 64 B
written per agent the source has recorded, 64 B written per agent only the destination has, 4 B per changed hot word, the
bit-plane words (16 B per tile read and written), the dense blocks and the source's queues; over 6.3 TB/s.
usage: python tools/filter_bench.py [--quick] [--logged | --params [--parent DIR] [--windows W] [--rounds N]] [--out PATH]"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (a worker of --logged imports the package of the tree it is told: --root DIR)
sys.path.insert(0, os.path.abspath(sys.argv[sys.argv.index('--root') + 1]) if '--root' in sys.argv[:-1] else ROOT)

from reina_model_amd import datasets, engine as eng, ensemble, filtering, snapshot as snapmod  # noqa: E402
from reina_model_amd.variables import VARIABLE_DEFAULTS  # noqa: E402

PEAK = 6.3e12


def sync():
    import torch
    torch.cuda.synchronize()


def timed(fn, reps):
    fn()
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), ts


def clone_bytes(contexts, pairs):
    """least bytes reina_group_clone moves for `pairs`, from the members' hot words and queue lengths"""
    n = contexts[0].engine.config.n_agents
    T = (n + 511) // 512
    hot = {}
    total, rec_src, only_dst = 0, 0, 0
    for d, s in pairs:
        for m in (d, s):
            if m not in hot:
                hot[m] = contexts[m].engine.tensors['hot'].cpu().numpy().view(np.uint32)
        hs, hd = hot[s], hot[d]
        rs = int(np.count_nonzero(hs))
        od = int(np.count_nonzero((hs == 0) & (hd != 0)))
        ch = int(np.count_nonzero(hs != hd))
        ql = contexts[s].engine.tensors['control'].cpu().numpy()[filtering.L_QUEUE0:filtering.L_QUEUE0 + 3]
        total += 8 * n + 128 * rs + 64 * od + 4 * ch + 2 * 2 * 64 * T \
            + 2 * 4 * (eng.COUNTER_WORDS + eng.L_NR + int(np.clip(ql, 0, None).sum()))
        rec_src += rs
        only_dst += od
    return total, rec_src, only_dst


def compare_routes(contexts, group, pairs, reps):
    """the clone of `pairs` against the snapshot route on the same list: ms (median), bytes.  Before every timed clone the
    destinations get their own states back (restores of images taken first, not timed), so each rep moves what a real
    resample moves."""
    disease = contexts[0]._disease
    nbytes, rec, od = clone_bytes(contexts, pairs)
    own = {d: snapmod.pack_engine(contexts[d].engine, disease, testing_ever=True) for d, _ in pairs}

    def reset():
        for d, img in own.items():
            snapmod.unpack_engine(contexts[d].engine, disease, img)
        sync()

    clone_ts = []
    for _ in range(reps + 1):
        reset()
        t0 = time.perf_counter()
        filtering.clone_group(group, pairs)
        sync()
        clone_ts.append((time.perf_counter() - t0) * 1e3)
    clone_ts = clone_ts[1:]
    clone_ms = float(np.median(clone_ts))
    srcs = sorted({s for _, s in pairs})

    def snap_route():
        imgs = {s: snapmod.pack_engine(contexts[s].engine, disease, testing_ever=True) for s in srcs}
        for d, s in pairs:
            snapmod.unpack_engine(contexts[d].engine, disease, imgs[s])

    snap_ms, snap_ts = timed(snap_route, reps)
    return dict(pairs=len(pairs), distinct_sources=len(srcs), clone_ms=clone_ms, clone_ms_all=clone_ts,
                snapshot_route_ms=snap_ms, snapshot_route_ms_all=snap_ts, speedup=snap_ms / clone_ms,
                clone_bytes=nbytes, recorded_in_sources=rec, recorded_only_in_destinations=od,
                clone_bytes_per_agent_pair=nbytes / len(pairs) / contexts[0].engine.config.n_agents,
                clone_model_ms_at_6p3=nbytes / PEAK * 1e3, clone_fraction_of_peak=nbytes / PEAK * 1e3 / clone_ms)


def case_hus(K, windows_cap, reps):
    import torch
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    obs = datasets.get_detected_cases('HUS')
    model = filtering.ObservationModel({'all_detected': 10.0, 'in_ward': 10.0})
    days = None if windows_cap is None else 7 * windows_cap
    t0 = time.perf_counter()
    r = filtering.particle_filter(v, K, observations=obs, obs_model=model, window=7, days=days, seeds=list(range(1, K + 1)),
                                  filter_seed=0)
    wall = time.perf_counter() - t0
    try:
        # the history read-back alone, on a block of one window's shape
        h = torch.zeros(K * 7 * eng.COUNTER_WORDS, dtype=torch.int32, device='cuda:0')
        rb_ms, _ = timed(lambda: r.contexts[0].engine.alloc.to_host(h), reps)
        per = []
        for w, t in zip(r.windows, r.timings):
            per.append(dict(start_day=w['start_day'], days=w['days'], ess=w['ess'], resampled=bool(w['resampled']),
                            pairs=t['pairs'], run_ms=t['run'] * 1e3, score_ms=t['score'] * 1e3,
                            resample_ms=t['resample'] * 1e3, clone_issue_ms=t['clone'] * 1e3))
        full = [p for p in per if p['days'] == 7]
        med = lambda k: float(np.median([p[k] for p in full]))
        last_pairs = None
        for w in reversed(r.windows):
            if w['resampled']:
                anc = w['ancestors']
                last_pairs = [(int(d), int(anc[d])) for d in range(K) if anc[d] != d]
                break
        routes = None
        if last_pairs:
            # (that resample's clone has made every destination its source: 7 more days under the members' own seeds first,
            # so the destinations differ from their sources as they do at a resample)
            r.forecast(7)
            routes = compare_routes(r.contexts, r.group, last_pairs, reps)
        return dict(case='hus_k128', K=K, agents=r.contexts[0].engine.config.n_agents, days=r.days, windows=len(r.windows),
                    resamples=int(sum(p['resampled'] for p in per)), wall_s=wall, log_evidence=r.log_evidence,
                    readback_ms_per_window=rb_ms,
                    median_window_ms=dict(run=med('run_ms'), days=med('run_ms') - rb_ms, readback=rb_ms, score=med('score_ms'),
                                          resample=med('resample_ms'), clone_issue=med('clone_issue_ms')),
                    windows_detail=per, last_resample_routes=routes)
    finally:
        r.close()


def log_clone_bytes(contexts, pairs, course):
    """bytes k_txlog_clone moves for `pairs` beyond the state's clone: (delta, dense)"""
    n = contexts[0].engine.config.n_agents
    hot = {m: contexts[m].engine.tensors['hot'].cpu().numpy().view(np.uint32) for pr in pairs for m in pr}
    either = sum(int(np.count_nonzero((hot[d] != 0) | (hot[s] != 0))) for d, s in pairs)
    per = 24 if course else 8
    return 8 * n * len(pairs) + per * either, per * n * len(pairs), either


def timed_clone(contexts, group, pairs, reps, log):
    """the synchronised clone of `pairs`, ms per rep; before every rep the destinations get their own states back (not timed),
    so each rep moves what a real resample moves (the log's launch moves the same bytes whatever the words hold)"""
    disease = contexts[0]._disease
    own = {d: snapmod.pack_engine(contexts[d].engine, disease, testing_ever=True) for d, _ in pairs}
    ts = []
    for _ in range(reps + 1):
        for d, img in own.items():
            snapmod.unpack_engine(contexts[d].engine, disease, img)
        sync()
        t0 = time.perf_counter()
        if log is None:
            filtering.clone_group(group, pairs)
        else:
            filtering.clone_group(group, pairs, log=log)
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts[1:]


LEGS = {'unlogged': {}, 'txlog': dict(txlog=True), 'course': dict(course=True)}
LOGGED_LEGS = ('unlogged', 'txlog', 'course')
PARAMS_LEGS = ('unlogged', 'params1', 'params4')


def params_space(n):
    """the first n of four knobs: the --params legs' parameter space"""
    from reina_model_amd.parameters import Knob, LogNormal, ParameterSpace
    knobs = [Knob('beta', 'infectiousness_multiplier', prior=LogNormal(1.0, 0.3), bounds=(0.25, 4.0)),
             Knob('severe', 'p_severe_given_symptomatic', prior=LogNormal(1.0, 0.2), bounds=(0.25, 4.0)),
             Knob('sus_old', 'p_susceptibility', ages=(60, 100), prior=LogNormal(1.0, 0.2), bounds=(0.25, 4.0)),
             Knob('incubation', 'mean_incubation_duration', prior=LogNormal(1.0, 0.1), bounds=(0.5, 2.0))]
    return ParameterSpace(knobs[:n])


def one_leg(leg, K, windows_cap, reps):
    """one leg of --logged / --params in this process: the HUS filter (wall time, synchronised at the end), 7 more days, the timed clone"""
    kw = dict(parameters=params_space(int(leg[6:]))) if leg.startswith('params') else LEGS[leg]
    logged = bool(kw.get('txlog') or kw.get('course'))
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    obs = datasets.get_detected_cases('HUS')
    model = filtering.ObservationModel({'all_detected': 10.0, 'in_ward': 10.0})
    days = None if windows_cap is None else 7 * windows_cap
    sync()
    t0 = time.perf_counter()
    r = filtering.particle_filter(v, K, observations=obs, obs_model=model, window=7, days=days, seeds=list(range(1, K + 1)),
                                  filter_seed=0, **kw)
    sync()
    wall = time.perf_counter() - t0
    try:
        run_ms = [t['run'] * 1e3 for t, w in zip(r.timings, r.windows) if w['days'] == 7]
        pairs = None
        for w in reversed(r.windows):
            if w['resampled']:
                anc = w['ancestors']
                pairs = [(int(d), int(anc[d])) for d in range(K) if anc[d] != d]
                break
        res = dict(leg=leg, agents=r.contexts[0].engine.config.n_agents, days=r.days, windows=len(r.windows),
                   resamples=int(sum(w['resampled'] for w in r.windows)), log_evidence=r.log_evidence, wall_s=wall,
                   wall_ms_per_window=sum(sum(t.get(k, 0.0) for k in ('run', 'score', 'resample', 'clone', 'params')) for t in r.timings) * 1e3 / len(r.windows),
                   median_window_run_ms=float(np.median(run_ms)))
        if pairs:
            r.forecast(7)   # (the destinations differ from their sources again, as they do at a resample)
            ts = timed_clone(r.contexts, r.group, pairs, reps, r.log if logged else None)
            res.update(pairs=len(pairs), clone_ms=float(np.median(ts)), clone_ms_all=ts)
            if logged:
                delta, dense, either = log_clone_bytes(r.contexts, pairs, 'course' in kw)
                res.update(log_bytes_delta=delta, log_bytes_dense=dense, recorded_in_either=either,
                           log_model_ms_at_6p3=delta / PEAK * 1e3)
        if leg.startswith('params'):
            # the synchronised set of all K members (the host mirrors and the launches), and the windows' own share
            from reina_model_amd.parameters import chunk
            dev, th = r.device_parameters, r.parameters
            ms, ts = timed(lambda: dev.set(range(K), th), reps)
            res.update(knobs=len(r.space), params_set_ms=ms, params_set_ms_all=ts, params_set_launches=-(-K // chunk(len(r.space))),
                       params_ms_per_resample=float(np.median([t['params'] * 1e3 for t, w in zip(r.timings, r.windows) if w['resampled']] or [0.0])),
                       final_theta_mean=[float(x) for x in (r.weights[:, None] * r.parameters).sum(axis=0)])
        return res
    finally:
        r.close()


def spread(xs):
    xs = [float(x) for x in xs]
    return dict(median=float(np.median(xs)), min=min(xs), max=max(xs), all=xs)


def case_logged(K, windows_cap, reps, parent, rounds, on_round=None, leg_names=LOGGED_LEGS, case='logged'):
    """every leg in a process of its own that imports the package of its tree (--leg, --root), the legs alternating round by
    round; `parent` (a built checkout of the parent commit) runs the unlogged leg as `parent_unlogged`"""
    import subprocess
    legs = [(name, ROOT) for name in leg_names]
    if parent:
        legs = [('parent_unlogged', os.path.abspath(parent))] + legs
    runs = {name: [] for name, _ in legs}

    def summary(rounds_done):
        out = dict(case='hus_k%d_%s' % (K, case), K=K, rounds=rounds_done, legs={})
        for name, rs in runs.items():
            last = {k: x for k, x in rs[-1].items() if k not in ('clone_ms_all', 'params_set_ms_all', 'leg')}
            if all('params_set_ms' in r for r in rs):
                last.update(params_set_ms=spread([r['params_set_ms'] for r in rs]), params_set_ms_last_round=rs[-1]['params_set_ms_all'])
            last.update(clone_ms=spread([r['clone_ms'] for r in rs]) if all('clone_ms' in r for r in rs) else None,
                        wall_ms_per_window=spread([r['wall_ms_per_window'] for r in rs]),
                        median_window_run_ms=spread([r['median_window_run_ms'] for r in rs]), wall_s=spread([r['wall_s'] for r in rs]),
                        clone_ms_last_round=rs[-1].get('clone_ms_all'))
            out['legs'][name] = last
        same = [rs for name, rs in runs.items() if not name.startswith('params')]   # (a prior changes the evidence)
        out['log_evidence_equal_in_every_leg' if len(same) == len(runs) else 'log_evidence_equal_without_parameters'] = \
            len({r['log_evidence'] for rs in same for r in rs}) == 1
        return out

    for rnd in range(rounds):
        for name, root in legs:
            cmd = [sys.executable, os.path.abspath(__file__), '--leg', name.replace('parent_', ''), '--root', root, '--reps', str(reps)]
            if windows_cap is not None:
                cmd += ['--windows', str(windows_cap)]
            out = subprocess.run(cmd, cwd=root, stdout=subprocess.PIPE, text=True, check=True).stdout
            runs[name].append(json.loads([ln for ln in out.splitlines() if ln.startswith('{"leg"')][-1]))
            print(json.dumps({name: {k: x for k, x in runs[name][-1].items() if k not in ('clone_ms_all', 'params_set_ms_all')}}), flush=True)
        if on_round is not None:
            on_round(summary(rnd + 1))   # (what has been measured so far is kept)
    return summary(rounds)


def case_1e7(n, K, days, reps):
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    ages = datasets.scaled_population(n)
    setup = ensemble.Setup(ages, ipc='auto')
    planner, ctxs = setup.planner(v, 1), setup.members(v, range(100, 100 + K))
    group, _ = ensemble.group_for(ctxs)
    try:
        t0 = time.perf_counter()
        ensemble.run_group_plan(ctxs, planner.make_plan(days), record_history=False, group=group)
        sync()
        run_s = time.perf_counter() - t0
        pairs = [(K // 2 + k, k) for k in range(K // 2)]
        out = dict(case='clone_1e7', agents=ctxs[0].engine.config.n_agents, K=K, day=days, group_days_s=run_s)
        out.update(compare_routes(ctxs, group, pairs, reps))
        return out
    finally:
        group.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--quick', action='store_true', help='4 HUS windows, 10^7 agents at day 60 (for the rocprofv3 run)')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'filter_bench.json'))
    ap.add_argument('--logged', action='store_true', help='the logged legs alone (profiles/filter_log_bench.json)')
    ap.add_argument('--params', action='store_true', help='the legs with per-particle parameters alone (profiles/params_bench.json)')
    ap.add_argument('--windows', type=int, default=None, help="--logged: so many 7-day windows (default: the case file's span)")
    ap.add_argument('--parent', default=None, help='--logged: a built checkout of the parent commit, for its unlogged leg')
    ap.add_argument('--rounds', type=int, default=3, help='--logged: rounds of the alternating legs')
    ap.add_argument('--leg', default=None, help='(a worker of --logged: this leg, in this process)')
    ap.add_argument('--root', default=ROOT, help='(a worker of --logged: the tree whose package it imports)')
    a = ap.parse_args()
    if a.leg:
        print(json.dumps(one_leg(a.leg, 128, a.windows, a.reps)), flush=True)
        return
    if a.logged or a.params:
        what = 'logged' if a.logged else 'params'
        out = a.out if a.out != ap.get_default('out') else os.path.join(ROOT, 'profiles', 'filter_log_bench.json' if a.logged else 'params_bench.json')

        def write(case):
            with open(out, 'w') as f:
                json.dump(dict(tool='tools/filter_bench.py --' + what, peak_bytes_per_s=PEAK, cases=[case]), f, indent=1)

        write(case_logged(128, a.windows, a.reps, a.parent, a.rounds, on_round=write,
                          leg_names=LOGGED_LEGS if a.logged else PARAMS_LEGS, case=what))
        return
    import torch
    res = dict(device=torch.cuda.get_device_name(0), peak_bytes_per_s=PEAK, cases=[])
    res['cases'].append(case_hus(128, 4 if a.quick else None, a.reps))
    print(json.dumps({k: v for k, v in res['cases'][-1].items() if k != 'windows_detail'}), flush=True)
    res['cases'].append(case_1e7(10_000_000, 16, 60 if a.quick else 120, a.reps))
    print(json.dumps(res['cases'][-1]), flush=True)
    if not a.quick or a.out != ap.get_default('out'):
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
