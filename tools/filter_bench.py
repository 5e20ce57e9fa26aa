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
Bytes of a clone, from the shapes and the recorded-agent counts: per pair 8 B per agent (both hot words), 64 B read + 64 B
written per agent the source has recorded, 64 B written per agent only the destination has, 4 B per changed hot word, the
bit-plane words (16 B per tile read and written), the dense blocks and the source's queues; over 6.3 TB/s.
usage: python tools/filter_bench.py [--quick] [--out PATH]"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from reina_model_amd import datasets, engine as eng, ensemble, filtering, simulation, snapshot as snapmod  # noqa: E402
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


def case_1e7(n, K, days, reps):
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    ages = datasets.scaled_population(n)
    planner = simulation.make_context(v, age_counts=ages, seed=1, ipc='auto')
    ctxs = [simulation.make_context(v, age_counts=ages, seed=100 + k, ipc='auto') for k in range(K)]
    group = eng.EngineGroup([c.engine for c in ctxs])
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
    a = ap.parse_args()
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
