"""Monte-Carlo ensembles: many independent simulations of the same scenario on one GPU.

Counterpart of the reference's `run_monte_carlo` (calc/simulation.py:349-385: a
`multiprocessing.Pool(8)` over seeds).  A single HUS-sized simulation keeps only a few per cent of
an MI355X busy (its day is a chain of short, latency-bound kernels), so an ensemble is run as K
engine instances side by side, every member owning its HBM state.  Two ways to issue the work:

  * batched (default): the members form an engine group (include/reina_hip.h: reina_group_*) and
    every phase of a day is ONE kernel launch covering all members (member = blockIdx.y) -- the
    launch count per day does not grow with K, so the host never becomes the limit;
  * threaded: every member has its own HIP stream and a small pool of host threads issues the
    members' days (the C ABI call releases the GIL); kept for members of differing scenarios.

Members are fully independent (BASELINE config 5: "replicas only", no collective); over several
GPUs the seeds are simply partitioned across ranks.  Results are bit-identical either way and
identical to running each seed alone (tests/test_parity_gpu.py).  How an ensemble is set up -- planner, members,
group -- is stated once, ahead of the routes (DESIGN.md "How an ensemble is set up").
"""
import ctypes
import os
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import (course as _crs, detection as _det, engine as _eng, lineage as _lin, policy as _pol, regime as _rgm, reports as _rep, simulation, snapshot as _snap,
               summary as _summ, transmission as _tx, txlog as _txl, vaccination as _vac)
from .dayrun import History, replay_plan
from .filtering import particle_filter  # noqa: F401  (conditioned ensembles: reina_model_amd/filtering.py)


class Setup:
    """What every Context of one ensemble is made with -- the same five keywords of simulation.make_context on every route --
    and, for the futures of one realised past, the snapshot.Snapshot they start from."""

    def __init__(self, age_counts=None, device='cuda:0', engine_factory=None, interventions=None, ipc=None, snapshot=None):
        self.kw = dict(age_counts=age_counts, device=device, engine_factory=engine_factory, interventions=interventions, ipc=ipc)
        self.snapshot = snapshot

    def context(self, variables, seed, disease=None, defer_ipc=False):
        """One member: a Context of `variables`; with a snapshot, restored on the HOST only (its checks and the scenario's
        state: the engines of all members are brought to it by one launch, restore_group).  `disease`: a ready disease block
        the member's engine is created with (run_parameter_ensemble on a library without reina_params.h); `defer_ipc`: the
        initial population condition waits for Context.apply_initial_condition (run_parameter_ensemble's device route)."""
        c = simulation.make_context(variables, seed=seed, disease=disease, defer_ipc=defer_ipc, **self.kw)
        if self.snapshot is not None:
            c.restore(self.snapshot, engine_state=False)
        return c

    def planner(self, variables, seed, policy=None):
        """A Context that only makes plans (its engine runs no day).  Under a policy the mask shares of the snapshot's last upload
        are replayed into it: the level tables start from them.  (particle_filter does without the replay: it takes no policy.)"""
        p = self.context(variables, seed)
        if policy is not None and self.snapshot is not None:
            p._packed_tables_for_restore(self.snapshot.state)
        return p

    def members(self, variables, seeds, member_variables=None):
        """One Context per seed, of `variables` or of member_variables[m]"""
        vs = member_variables if member_variables is not None else [variables] * len(seeds)
        return [self.context(v, sd) for v, sd in zip(vs, seeds)]

    def restore_group(self, group, contexts):
        """Brings the group of `contexts` to the snapshot, when there is one: the image unpacked into all members by one launch
        (reina_group_snap_unpack), then every member's contact tables as of the snapshot's day."""
        if self.snapshot is not None:
            _snap.unpack_group(group, contexts[0]._disease, self.snapshot.image)
            for c in contexts:
                c.engine.upload_contact_tables(*c._packed_tables_for_restore(self.snapshot.state))


def group_for(contexts, group=None, route=None):
    """(group, made here): the caller's `group`, checked to be that of exactly these contexts' engines, or one made here"""
    if group is None:
        return _eng.EngineGroup([c.engine for c in contexts]), True
    if [e._h.value for e in group.engines] != [c.engine._h.value for c in contexts]:
        raise ValueError('%s: `group` is not the group of these contexts' % route)
    return group, False


def check_shared_days(plans, what):
    """Plans that share a group share their day descriptors: refuses the first `what` ('scenario', 'branch') whose plan differs
    from plan 0 in them.  (Plans that are the same object need no look.)"""
    words = lambda p: [(n, ctypes.string_at(a, ctypes.sizeof(a))) for _, a, n in p['segments']]
    for k, p in enumerate(plans[1:], 1):
        if p is not plans[0] and words(p) != words(plans[0]):
            raise ValueError('%s %d differs from %s 0 in more than the values of its mobility / mask '
                             'interventions: it cannot share a group' % (what, k, what))


def plan_once(setup, variables, seed, days, summary=None):
    """(plan, pending) of a run in chunks of members: the plan, made ONCE by a planner that goes at once -- the day descriptors
    do not depend on the seed --, and with `summary` (summary.SummarySpec) the summary.Pending of the chunks' rows, else None"""
    planner = setup.planner(variables, seed)
    plan = planner.make_plan(days)
    return plan, (_summ.Pending(summary, planner, plan['start_day']) if summary is not None else None)


def chunks(seeds, size):
    return [seeds[start:start + size] for start in range(0, len(seeds), size)]


def _stopwatch(route):
    """REINA_ENS_TIMING (diagnostic: tools/ens_first_run2.py): mark(name) takes the time, the last prints where the time went"""
    marks = [('start', time.perf_counter())] if os.environ.get('REINA_ENS_TIMING') else None

    def mark(name, last=False):
        if marks is not None:
            marks.append((name, time.perf_counter()))
            if last:
                print(route + ': ' + ' | '.join('%s %.1f ms' % (n, (t - marks[k][1]) * 1e3) for k, (n, t) in enumerate(marks[1:])), flush=True)
    return mark


def _refuse_group_plan(contexts, plan, record_history, member_plans, policy, txlog, summary):
    """what run_group_plan refuses before anything runs"""
    if summary is not None:
        _summ.check_group(summary, contexts, plan, record_history)
    logged = [c.transmission_log is not None for c in contexts]
    if any(logged) and not all(logged):
        raise ValueError('run_group_plan: some members keep a transmission log and some do not')
    if policy is not None:
        if member_plans is not None:
            raise ValueError('run_group_plan: a policy and member_plans (a sweep) cannot be combined')
        if (txlog or any(logged)) and contexts and getattr(contexts[0].engine, 'regime_f', None) is None:
            raise ValueError('run_group_plan: a transmission log and a policy cannot be combined on this engine library (it lacks '
                             'the combined run of include/reina_regime.h)')
        if plan.get('policy') is not policy or plan.get('policy_banks') is None:
            raise ValueError('run_group_plan: the plan must be made with the policy (make_plan(days, policy=...))')
        for c in contexts:
            _pol.check_capable(c)


def _group_and_log(contexts, group, txlog, course):
    """(group, made here, the group's txlog.DeviceLog or None): the group of a logged group's log when none is given (the log
    keeps its group open), else group_for; the members' log continued, or begun with `txlog`."""
    logged = bool(contexts) and contexts[0].transmission_log is not None   # (all or none: _refuse_group_plan)
    if group is None and logged and contexts[0].transmission_log.device is not None:
        group = contexts[0].transmission_log.device.group
    group, own_group = group_for(contexts, group, 'run_group_plan')
    for c in contexts:
        c._replayed = True
    glog = _rep.shared_log(contexts, group, "run_group_plan: the members' transmission logs are not those of this group (logs "
                           'begun one by one, or with another group, cannot be continued as a group)') if logged else None
    if glog is not None or txlog:
        glog = _txl.attach_group(contexts, group, glog, course)
    return group, own_group, glog


def _replay_group_plan(contexts, plan, member_plans, group, glog, policy, hist):
    """The plan's days issued to the group -- through the policy.DevicePolicy of a policy (returned, else None; it records
    into the group's log when there is one), through the group's log, or to the group itself; a sweep's members get their own
    tables at every table change."""
    if policy is not None:
        dev = _pol.DevicePolicy(policy, contexts[0].start_date, group=group)
        dev.log = glog
        replay_plan(plan, dev, hist, lambda si, tables: dev.upload_bank(plan['policy_banks'][si][0]))
        return dev

    def upload_member_tables(si, tables):   # (a sweep: every member its own)
        for c, mp in zip(contexts, member_plans):
            if mp['segments'][si][0] is not None:
                c.engine.upload_contact_tables(*mp['segments'][si][0])

    def upload_group_tables(si, tables):
        if tables is not None:
            group.upload_contact_tables(*tables)

    replay_plan(plan, glog if glog is not None else group, hist, upload_member_tables if member_plans is not None else upload_group_tables)


def _end_group_plan(contexts, plan, member_plans, dev, hist, summary, alloc, mark):
    """The members' end: under a policy (dev) their levels from the trace (the run's wait; their host-side table mirrors follow
    them), their day and mobility factors, the history or its summary (returned), and SimulationFailed for a problem word."""
    days, start_day = plan['days'], plan['start_day']
    if dev is not None:
        trace = dev.read_trace(start_day, days)
        dev.close()
        seg_of_day, factors = _pol.plan_segments_of_days(plan), [b[1] for b in plan['policy_banks']]
    for m, c in enumerate(contexts):
        if dev is not None:
            _pol._end_device_run(c, trace, m, start_day, plan['mobility_history'][0] if days else 0.0, seg_of_day, factors)
        else:
            c.mobility_history = (member_plans[m] if member_plans is not None else plan)['mobility_history']
        c.day = start_day + days
    out = hist.to_host() if summary is None else _summ.of_group(summary, hist.rows(), contexts, start_day)
    mark('history on the host')
    torch = getattr(alloc, 'torch', None)
    # on the device the members' final counter blocks (the problem word among them) in one copy instead of one per member (4 ms for 128)
    finals = (alloc.to_host(torch.stack([c.engine.tensors['counters'] for c in contexts])) if torch is not None else
              [c.engine.read_counters() for c in contexts])
    for c, final in zip(contexts, finals):
        c._raise_on_problem(np.asarray(final))
    mark('final counters')
    return out


def run_group_plan(contexts, plan, record_history=True, member_plans=None, group=None, policy=None, txlog=False, summary=None, course=False):
    """Execute `plan` (Context.make_plan) for all `contexts` as one engine group.  Returns
    history[len(contexts), days, COUNTER_WORDS] (host) or None.

    `member_plans` (one plan per context, see run_sweep): an intervention sweep -- the members' scenarios
    differ in the VALUES of their mobility limits / mask shares only, so they share the day descriptors
    of `plan` while every member gets its own contact tables at each table change.

    `group`: an engine.EngineGroup of exactly these contexts' engines, made by the caller (run_branches restores its members
    with one launch first); it stays open.  Otherwise a group is made for the run and closed after it.

    `policy` (policy.Policy; the plan made with it, make_plan(days, policy=...)): every member reacts to its own counters --
    k_policy ahead of every day, one bank of level tables for the whole group.  Every member starts at level 0 with an empty
    ring; its levels end up in `context.policy_levels`, its mobility factors in `context.mobility_history`.

    `txlog`: every member keeps a dated transmission log (reina_model_amd/txlog.py), recorded by one launch a day for the
    whole group; the members' logs end up on `contexts[m].transmission_log` and share the group's device log, which lives as
    long as they do (and keeps a group made for the run open).  A later call with the same `group` continues them; members that keep logs already are continued
    whatever `txlog` says.  Together with a policy: the record launch comes behind every day of the policy run
    (include/reina_regime.h), and regime_reports(contexts) reports transmission by every member's own levels.

    `course`: every member keeps a clinical course log too (reina_model_amd/course.py), attached to the group's transmission
    log and recorded by the same launch; implies `txlog`.  The members' course logs end up on `contexts[m].course_log`
    (course_reports(contexts): one launch for all).

    `summary` (summary.SummarySpec): an EnsembleSummary (quantile bands, peaks, exceedance: reina_model_amd/summary.py) is
    returned in place of the history, computed where the rows are: a device group's rows are never read back.  The members'
    final counters are checked as always."""
    txlog = txlog or course
    _refuse_group_plan(contexts, plan, record_history, member_plans, policy, txlog, summary)
    mark = _stopwatch('run_group_plan')
    group, own_group, glog = _group_and_log(contexts, group, txlog, course)
    hist = History(plan['days'], record_history, group=group)
    dev = _replay_group_plan(contexts, plan, member_plans, group, glog, policy, hist)
    mark('issued')
    out = _end_group_plan(contexts, plan, member_plans, dev, hist, summary, group.alloc, mark)
    if own_group and glog is None:   # (a group made here for a logged run stays open with its log, and goes with it)
        group.close()
    mark('closed', last=True)
    return out


def run_sweep(variables_list, seeds, days, age_counts=None, device='cuda:0', engine_factory=None, ipc='auto'):
    """BASELINE config 5's "intervention sweep": member m runs scenario variables_list[m] with seed
    seeds[m], all as ONE engine group.  The scenarios must agree in everything that goes into the day
    descriptors (dates, testing modes, imports, vaccination, capacities) and in the dates of their
    limit-mobility / wear-masks interventions; they may differ in those interventions' values (each member
    gets its own contact tables).  Returns (history[len(seeds), days, COUNTER_WORDS], contexts)."""
    assert len(variables_list) == len(seeds)
    setup = Setup(age_counts, device, engine_factory, None, ipc)
    plans = [setup.planner(v, sd).make_plan(days) for v, sd in zip(variables_list, seeds)]
    ctxs = setup.members(None, seeds, variables_list)
    check_shared_days(plans, 'scenario')
    return run_group_plan(ctxs, plans[0], member_plans=plans), ctxs


def run_ensemble_distributed(variables, seeds, days, group=None, concurrent=64, **kw):
    """BASELINE config 5: an ensemble over the GPUs of a node.  Replicas only -- rank r of the
    torch.distributed group runs seeds[r::world] as engine groups on its own GPU, no data-path
    collective; the histories are gathered on rank 0 (returned there in seed order, None elsewhere)."""
    import torch.distributed as dist
    seeds = list(seeds)
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    mine = seeds[rank::world]
    hist = run_ensemble(variables, mine, days, concurrent=concurrent, **kw) if mine else None
    parts = [None] * world if rank == 0 else None
    dist.gather_object((mine, hist), parts, dst=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
    if rank != 0:
        return None
    by_seed = {sd: h[k] for sds, h in parts for k, sd in enumerate(sds)}
    return np.stack([by_seed[sd] for sd in seeds])


def run_ensemble(variables, seeds, days, age_counts=None, device='cuda:0', threads=8, concurrent=None,
                 interventions=None, batched=True, engine_factory=None, ipc='auto', summary=None):
    """Run one simulation per seed for `days` days. Returns history[len(seeds), days, COUNTER_WORDS]
    (row d = counters before day d, as Context.run). `concurrent` bounds how many members hold HBM
    state at once (default: all).  `ipc`: the initial population condition of every member; 'auto' = the
    one simulate_individuals applies for these variables (calc/simulation.py:152), None = none.
    `summary` (summary.SummarySpec): the EnsembleSummary of all seeds instead of the history -- the chunks' histories stay on
    the device until the last has run and are summarised in one call; the threaded route summarises on the host."""
    seeds = list(seeds)
    concurrent = len(seeds) if concurrent is None else max(1, int(concurrent))
    # (the threaded route has always made its Contexts with the library's own engines: `engine_factory` is the batched route's)
    setup = Setup(age_counts, device, engine_factory if batched else None, interventions, ipc)
    plan, pending = plan_once(setup, variables, seeds[0], days, summary)
    if batched:
        outs = [run_group_plan(setup.members(variables, part), plan, summary=pending) for part in chunks(seeds, concurrent)]
    else:
        outs = [_run_threaded(setup, variables, part, plan, device, threads) for part in chunks(seeds, concurrent)]
        if pending is not None:
            pending.add(np.concatenate(outs))
    return pending.finish(members=seeds) if pending is not None else np.concatenate(outs)


def _run_threaded(setup, variables, seeds, plan, device, threads):
    """history [len(seeds), days, COUNTER_WORDS] of the members of `seeds`, each on a HIP stream of its own, their days issued
    by a pool of host threads"""
    import torch
    dev = torch.device(device)
    lock = threading.Lock()

    def work(seed):
        torch.cuda.set_device(dev)
        stream = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(stream):
            with lock:  # context construction touches shared Python state (allocator, caches)
                ctx = setup.context(variables, seed)
            hist = ctx.run_plan(plan)
            stream.synchronize()
        return hist

    with ThreadPoolExecutor(max_workers=min(threads, len(seeds))) as pool:
        return np.stack(list(pool.map(work, seeds)))


def run_policy_ensemble(variables, seeds, days, policy, age_counts=None, device='cuda:0', engine_factory=None, ipc='auto',
                        interventions=None, summary=None, txlog=False, course=False):
    """One simulation per seed for `days` days, every member reacting to its own counters under `policy` (policy.Policy), all
    as ONE engine group.  Returns (history[K, days, COUNTER_WORDS], levels[K, days], contexts).  An engine library without the
    policy entry points runs the members one after the other by policy.run_host_driven.  `summary` (summary.SummarySpec): the
    EnsembleSummary in place of the history.  `txlog` / `course`: every member keeps a dated transmission log / a clinical
    course log too (run_group_plan; on the host-driven route each member keeps its own in host memory)."""
    seeds = list(seeds)
    setup = Setup(age_counts, device, engine_factory, interventions, ipc)
    ctxs = setup.members(variables, seeds)   # (ahead of the planner: what the members' library can do decides whether there is one)
    if ctxs[0].engine.policy_f is None:
        for c in ctxs:
            if txlog or course:
                c.start_transmission_log()
            if course:
                c.start_course_log()
        hist = np.stack([_pol.run_host_driven(c, policy, days) for c in ctxs])
        if summary is not None:
            hist = _summ.summarise(hist, ctxs[0].nr_ages, summary, ctx=ctxs[0], members=seeds)
    else:
        plan = setup.planner(variables, seeds[0]).make_plan(days, policy=policy)
        hist = run_group_plan(ctxs, plan, policy=policy, summary=summary, txlog=txlog, course=course)
    return hist, np.stack([c.policy_levels for c in ctxs]), ctxs


def run_parameter_ensemble(variables, thetas, seeds, days, space, summary=None, age_counts=None, device='cuda:0',
                           engine_factory=None, ipc='auto', interventions=None):
    """The static case of per-member disease parameters (reina_model_amd/parameters.py): member m runs `days` days of
    `variables` with seed seeds[m] under row m of `thetas` ([K, P], one column per knob of the parameters.ParameterSpace
    `space`), all as ONE engine group -- prior-predictive runs, sensitivity sweeps.  On the device the members are made with
    the scenario's disease and one launch (reina_group_params_set) expands all K rows before day 0; on an engine library
    without the entry points every member is instead CREATED with parameters.expand_numpy's block.  Both routes leave the
    same blocks, and every member's Context._disease is its own.  Returns (history[K, days, COUNTER_WORDS], contexts);
    with `summary` (summary.SummarySpec) the EnsembleSummary in place of the history."""
    from . import parameters as _par
    seeds = list(seeds)
    setup = Setup(age_counts, device, engine_factory, interventions, ipc)
    planner = setup.planner(variables, seeds[0])
    base, A, V = planner._disease, planner.nr_ages, planner.nr_variants
    thetas = np.asarray(thetas, dtype=np.float32).reshape(len(seeds), len(space))
    blocks = _par.expand_many(base, space, thetas, A, V)
    plan = planner.make_plan(days)
    if planner.engine.params_f is None:
        ctxs = [setup.context(variables, sd, disease=b) for sd, b in zip(seeds, blocks)]
        return run_group_plan(ctxs, plan, summary=summary), ctxs
    # (the initial population condition draws durations and severities from the disease: it is applied behind the set, so that
    # it is drawn under the member's own block as on the other route)
    ctxs = [setup.context(variables, sd, defer_ipc=True) for sd in seeds]
    group, _ = group_for(ctxs)
    try:
        dev = _par.DeviceParameters(group, base, space)
        try:
            dev.set(range(len(seeds)), thetas)
            for c, b in zip(ctxs, blocks):
                c._disease = b
                c.apply_initial_condition()
            hist = run_group_plan(ctxs, plan, group=group, summary=summary)
        finally:
            dev.close()
    finally:
        group.close()
    return hist, ctxs


def run_branches(snap, variables, seeds, days, member_variables=None, age_counts=None, device='cuda:0', engine_factory=None,
                 interventions=None, policy=None, summary=None):
    """Conditional ensemble: K = len(seeds) futures of ONE realised past.  Every member is a Context of `variables` (or of
    member_variables[m]) restored from `snap` (snapshot.Snapshot) -- on the device all K by one launch
    (reina_group_snap_unpack) -- with its own seed, then `days` days are run as one engine group (run_group_plan).
    member_variables follows run_sweep's rule: the members may differ only in the values of their mobility and mask
    interventions.  `interventions`: intervention tuples of every member instead of its variables' scenario (make_context).
    `policy` (policy.Policy): every future reacts to its own course from the snapshot's day on (levels in
    contexts[m].policy_levels); not together with member_variables.
    Returns (history[K, days, COUNTER_WORDS], contexts); with `summary` (summary.SummarySpec) the EnsembleSummary of the futures
    in place of the history."""
    if policy is not None and member_variables is not None:
        raise ValueError('run_branches: a policy and member_variables cannot be combined')
    vs = list(member_variables) if member_variables is not None else [variables] * len(seeds)
    if len(vs) != len(seeds):
        raise ValueError('run_branches: one member_variables entry per seed')
    setup = Setup(age_counts, device, engine_factory, interventions, None, snapshot=snap)
    plans = []
    for v, sd in zip(vs, seeds):   # (one planner per distinct variables)
        plans.append(plans[0] if plans and v is vs[0] else setup.planner(v, sd, policy).make_plan(days, policy=policy))
    check_shared_days(plans, 'branch')
    ctxs = setup.members(None, seeds, vs)
    group, _ = group_for(ctxs)
    try:
        setup.restore_group(group, ctxs)
        hist = run_group_plan(ctxs, plans[0], member_plans=plans if member_variables is not None else None, group=group,
                              policy=policy, summary=summary)
    finally:
        group.close()
    return hist, ctxs


def transmission_reports(contexts, age_groups=None, group=None):
    """Context.transmission_report of every context, between the same two days: the members' reports as ONE launch per pass on
    the device (reina_group_tx_report), one report per member for host-memory engines.  `group`: an engine.EngineGroup of
    exactly these contexts' engines (stays open); otherwise one is made for the call and closed after it."""
    contexts = list(contexts)
    for c in contexts:
        c._check_tx_capable()
    table, labels = contexts[0]._tx_groups(age_groups)
    if not _eng.is_device(contexts[0].engine):
        reps = [_tx.report_engine(c.engine, table, len(labels)) for c in contexts]
    else:
        group, own_group = group_for(contexts, group, 'transmission_reports')
        try:
            reps = _tx.report_group(group, table, len(labels))
        finally:
            if own_group:
                group.close()
    for r in reps:
        r.group_labels = labels
    return reps


# The reports of a log, of every context between the same two days (reports.reports_of_contexts): the members of a logged group
# (run_group_plan(..., txlog=True[, course=True])) by ONE launch -- one per pass for the lineage report --, contexts that keep
# logs of their own, and engine libraries without the report's entry points, one by one.

def log_reports(contexts, age_groups=None, n_days=None):
    """txlog.LogReport of every context (one launch: reina_group_txlog_report)"""
    return _rep.reports_of_contexts(_txl.LOG, contexts, age_groups, n_days)


def lineage_reports(contexts, period=7, n_periods=None, age_groups=None):
    """lineage.LineageReport of every context (one launch per pass: reina_group_lineage_report)"""
    return _rep.reports_of_contexts(_lin.LINEAGE, contexts, period, n_periods, age_groups)


def course_reports(contexts, age_groups=None, n_days=None):
    """course.CourseReport of every context (one launch: reina_course_report)"""
    return _rep.reports_of_contexts(_crs.COURSE, contexts, age_groups, n_days)


def vaccination_reports(contexts, age_groups=None, n_days=None):
    """vaccination.VaccinationReport of every context (one launch: reina_vacc_report)"""
    return _rep.reports_of_contexts(_vac.VACCINATION, contexts, age_groups, n_days)


def regime_reports(contexts, labels=None, age_groups=None, n_days=None):
    """regime.RegimeReport of every context (one launch: reina_group_regime_report), each member with labels of its own: one
    sequence per context, or None for every context's own policy levels (Context.policy_level_by_day)"""
    return _rgm.report_contexts(contexts, labels, age_groups, n_days)


def detection_reports(contexts, age_groups=None, n_days=None):
    """detection.DetectionReport of every context (one launch: reina_detect_report); the contexts keep course logs"""
    return _rep.reports_of_contexts(_det.DETECTION, contexts, age_groups, n_days)
