"""Vaccination-report timings on one GPU.  Writes profiles/vaccination_bench.json (or --out).  Kernel times come from a separate
run of this script under `rocprofv3 --kernel-trace --stats` (`--quick`; profiles/vaccination_kernel_stats.csv).

Two scenarios, each run once with txlog=True and course=True (the course report of the same state is the yardstick: same
stream of hot and log words, and k_course_report reads a record where k_vacc_report reads a vaccinated agent's cold sector):
  hus      HUS x 365 days with a mass programme (350 000 doses a week for everybody from 16 up, from day 10)
  turku    the Turku override set, scenario `astra-zeneca` (['vaccinate', '2021-03-15', 2000, 25, 55]) x 470 days
Timed, medians of --reps calls with min and max, the first call apart:
  report        ctx.transmission_log.vaccination_report() as a user calls it: launch, wait, read-back, the Report object
  course        ctx.course_log.report() the same way
  numpy         vaccination.report_numpy on the read-back state (hot, vacc_day, log words); the read-back is timed beside it
The realised protection the scenario shows -- by age group: severe share and death share of the protected and of the
unvaccinated, with their counts -- goes into the file too: it is a result of the model, the same on every engine.
usage: python tools/vaccination_bench.py [--reps N] [--quick] [--only hus|turku] [--out PATH]"""
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


def scenarios():
    from reina_model_amd.variables import HUS_DEFAULTS, copy_variables
    hus = copy.deepcopy(HUS_DEFAULTS)
    hus['interventions'] = list(hus['interventions']) + [['vaccinate', '2020-02-28', 350000, 16, 100]]
    return dict(hus=(hus, 365), turku=(copy_variables(override_set='turku', active_scenario='astra-zeneca'), 470))


def spread(ts):
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts), n=len(ts))


def timed(fn, reps):
    ts = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, dict(spread(ts[1:]), first_ms=ts[0])


def protection(r):
    out = []
    for g, label in enumerate(r._groups()):
        s, d = r.protection_against_severe(g), r.protection_against_death(g)
        out.append(dict(group=label, recent=int(r.outcome[1, g, 0]), severe=s._asdict(), death=d._asdict()))
    out.append(dict(group='all', recent=int(r.outcome[1, :, 0].sum()), severe=r.protection_against_severe()._asdict(),
                    death=r.protection_against_death()._asdict()))
    return out


def run(name, reps, quick):
    import numpy as np
    from reina_model_amd import simulation, vaccination as vac
    v, days = scenarios()[name]
    ctx = simulation.make_context(v, seed=1, ipc='auto', txlog=True, course=True)
    t0 = time.perf_counter()
    ctx.run(days)
    run_ms = (time.perf_counter() - t0) * 1e3
    tlog = ctx.transmission_log
    if quick:
        tlog.vaccination_report()
        ctx.course_log.report()
        return None
    rep, t_rep = timed(tlog.vaccination_report, reps)
    _, t_course = timed(ctx.course_log.report, reps)

    def read_back():
        hot = ctx.engine.tensors['hot'].cpu().numpy().view(np.uint32)
        return hot, ctx.engine.tensors['vacc_day'].cpu().numpy(), tlog.words()

    (hot, vd, log), t_read = timed(read_back, reps)
    table = ctx._tx_groups(None)[0]
    spec, t_numpy = timed(lambda: vac.report_numpy(hot, vd, log, ctx.age_start, table, days), reps)
    assert np.array_equal(spec.words, rep.words), 'the device report differs from report_numpy of the read-back state'
    n = int(ctx.engine.config.n_agents)
    # a report's least bytes: the hot word of every agent, the log word of every infected one, one 32-byte sector of every vaccinated one
    least = 4.0 * n + 4.0 * rep.infected + 32.0 * rep.vaccinated
    scalars = {k: int(getattr(rep, k)) for k in vac.SCALAR_NAMES}
    return dict(n_agents=n, days=days, run_ms=run_ms, report=t_rep, course_report=t_course, read_back=t_read, numpy=t_numpy,
                report_words=int(vac.report_words(days)), scalars=scalars, least_bytes=least, least_bytes_at_hbm_rate_us=least / HBM * 1e6,
                by_status=[int(x) for x in rep.outcome[:, :, 0].sum(axis=1)], coverage_last_day=[float(x) for x in rep.coverage_frame().iloc[-1]],
                protection=protection(rep))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--quick', action='store_true', help='for the rocprofv3 run: each scenario once, one vaccination report and one course report')
    ap.add_argument('--only', choices=('hus', 'turku'), default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vaccination_bench.json'))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('vaccination_bench: no GPU visible; timings are taken on the device only')
    res = dict(device=torch.cuda.get_device_name(0), tool='tools/vaccination_bench.py')
    for name in ('hus', 'turku') if a.only is None else (a.only,):
        r = run(name, a.reps, a.quick)
        if r is not None:
            res[name] = r
            print(json.dumps({name: dict(report=r['report'], course_report=r['course_report'], numpy=r['numpy'], scalars=r['scalars'])}), flush=True)
    if not a.quick and a.out and a.out != os.devnull:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
