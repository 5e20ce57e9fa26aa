"""Detection-report timings on one GPU.  Writes profiles/detection_bench.json (or --out).  Kernel times come from a separate run
of this script under `rocprofv3 --kernel-trace --stats` (`--quick`; profiles/detection_kernel_stats.csv): the three reports once
with n_days = 365 (a kernel's MaxNs) and once with n_days = 1, where no day is in range and no table by day is written (MinNs).

One scenario: HUS x 365 days under the default interventions (they hold testing and tracing), run once with course=True.  The
yardstick is the course report plus the log report of the same state: k_detect_report reads the union of what k_course_report
and k_txlog_report read, plus one gathered record per link.
Timed, medians of --reps calls with min and max, the first call apart:
  report        ctx.course_log.detection_report() as a user calls it: launch, wait, read-back, the Report object
  course        ctx.course_log.report() the same way
  log           ctx.transmission_log.report() the same way
  numpy         detection.report_numpy on the read-back state (hot, cold, log words, records); the read-back is timed beside it
The tool asserts that the device report equals report_numpy word for word.  What the scenario shows -- ascertainment, the share of
transmission from never-detected agents, lead times, pairs -- goes into the file too: a result of the model, the same on every engine.
usage: python tools/detection_bench.py [--reps N] [--quick] [--out PATH]"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
HBM = 6.3e12   # bytes a second: tools/txlog_bench.py's, the rate the other benches state their fractions of
DAYS = 365


def spread(ts):
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts), n=len(ts))


def timed(fn, reps):
    ts = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, dict(spread(ts[1:]), first_ms=ts[0])


def findings(r):
    share = lambda s: dict(share=s.share, count=s.count, total=s.total)
    al, lt, pr = r.days_at_large(), r.lead_time(), r.pair_detection()
    return dict(ascertained_share=(r.infected - r.never) / r.infected if r.infected else None,
                by_phase=[int(x) for x in r.phase.sum(axis=0)], link_classes=[int(x) for x in r.link_class.sum(axis=0)],
                transmission_never=share(r.transmission_share('never')), transmission_never_closed=share(r.transmission_share('never', closed_only=True)),
                days_at_large_mean=al.mean(), lead_mean=lt.mean(), averted_if_1_day_earlier=share(r.averted_if_earlier(1)),
                averted_if_3_days_earlier=share(r.averted_if_earlier(3)), dated_pairs=pr.total(), adjacent_share_1=r.adjacent_share(1))


def run(reps, quick):
    import numpy as np
    from reina_model_amd import detection as det, reports
    from reina_model_amd import simulation
    from reina_model_amd.variables import HUS_DEFAULTS
    ctx = simulation.make_context(copy.deepcopy(HUS_DEFAULTS), seed=1, ipc='auto', course=True)
    t0 = time.perf_counter()
    ctx.run(DAYS)
    run_ms = (time.perf_counter() - t0) * 1e3
    course, tlog = ctx.course_log, ctx.transmission_log
    if quick:
        for n_days in (DAYS, 1):            # (with n_days = 1 no known day is in range: the kernels without their tables by day)
            course.detection_report(n_days=n_days)
            course.report(n_days=n_days)
            tlog.report(n_days=n_days)
        return None
    rep, t_rep = timed(course.detection_report, reps)
    _, t_course = timed(course.report, reps)
    _, t_log = timed(tlog.report, reps)

    def read_back():
        hot, infector, n_infected, _ = reports.host_state(ctx.engine)
        return hot, infector, n_infected, tlog.words(), course.words()

    state, t_read = timed(read_back, reps)
    table = ctx._tx_groups(None)[0]
    spec, t_numpy = timed(lambda: det.report_numpy(*state, ctx.age_start, table, DAYS), reps)
    assert np.array_equal(spec.words, rep.words), 'the device report differs from report_numpy of the read-back state'
    n = int(ctx.engine.config.n_agents)
    # a report's least bytes (an estimate from the shapes): hot and log word of every agent, a 32-byte sector of the cold record
    # and of the course record of every infected one, and three more sectors (hot, log, record of the infector) of every link
    least = 8.0 * n + 64.0 * rep.infected + 96.0 * rep.linked
    scalars = {k: int(getattr(rep, k)) for k in det.SCALAR_NAMES}
    return dict(n_agents=n, days=DAYS, run_ms=run_ms, report=t_rep, course_report=t_course, log_report=t_log, read_back=t_read, numpy=t_numpy,
                report_words=int(det.report_words(DAYS)), scalars=scalars, least_bytes=least, least_bytes_at_hbm_rate_us=least / HBM * 1e6,
                findings=findings(rep))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--quick', action='store_true', help='for the rocprofv3 run: the scenario once, then the detection, course and log report with n_days 365 and 1')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'detection_bench.json'))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('detection_bench: no GPU visible; timings are taken on the device only')
    res = dict(device=torch.cuda.get_device_name(0), tool='tools/detection_bench.py')
    r = run(a.reps, a.quick)
    if r is not None:
        res['hus'] = r
        print(json.dumps(dict(report=r['report'], course_report=r['course_report'], log_report=r['log_report'], numpy=r['numpy'],
                              read_back=r['read_back'], scalars=r['scalars'], findings=r['findings'])), flush=True)
    if not a.quick and a.out and a.out != os.devnull:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
