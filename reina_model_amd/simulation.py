"""Driver with the contract of the reference's `calc/simulation.py:17-290`.

`simulate_individuals(variables)` builds the population / healthcare / disease parameter dicts the
same way (`create_disease_params` :50-61, `make_age_groups` :103-116), constructs the engine
`Context`, runs the day loop and returns the same two DataFrames `(df, adf)`:
  df  : one row per date, columns POP_ATTRS + STATE_ATTRS + EXPOSURES_ATTRS + ['us_per_infected']
  adf : per-date x (attr, age group) population counts.
Row d is the state BEFORE day d is simulated (the reference calls generate_state() before
iterate(), :195 vs :270).  The day loop itself runs on the GPU without per-day host round trips
(`Context.run`); `step_callback` is honoured every `callback_day_interval` days by running the
simulation in stretches.

Also here, with the reference's names: `sample_model_parameters` (:301-347), `simulate_monte_carlo`
/ `run_monte_carlo` (:350-385; the reference maps 1000 seeds over a pool of 8 processes, here the
seeds run as engine groups on the GPU, reina_model_amd/ensemble.py) and the `python -m` day table
(:388-460): `python -m reina_model_amd.simulation [--days N] [--seed S] [--scenario ID]`.
"""
import time
from datetime import date, timedelta

import numpy as np

from . import datasets
from . import engine as _eng
from . import model
from .interventions import get_active_interventions, iv_tuple_to_obj
from .variables import copy_variables

POP_ATTRS = ['susceptible', 'vaccinated', 'infected', 'detected', 'all_detected', 'in_ward', 'in_icu',
             'dead', 'non_hospital_deaths', 'recovered', 'all_infected', 'new_infections']
EXPOSURES_ATTRS = ['exposures_home', 'exposures_work', 'exposures_school', 'exposures_transport',
                   'exposures_leisure', 'exposures_other']
STATE_ATTRS = ['exposed_per_day', 'available_hospital_beds', 'available_icu_units', 'total_icu_units',
               'ct_cases_per_day', 'r', 'mobility_limitation']


class ExecutionInterrupted(Exception):
    pass


def create_disease_params(variables):
    """calc/simulation.py:50-61: every p_* / ratio_* variable is a percentage."""
    kwargs = {}
    for key in model.DISEASE_PARAMS:
        val = variables[key]
        if key.startswith('p_') or key.startswith('ratio_'):
            if isinstance(val, list):
                val = [(age, sev / 100) for age, sev in val]
            else:
                val = val / 100
        kwargs[key] = val
    return kwargs


def make_context(variables, age_counts=None, seed=None, interventions=None, device='cuda:0',
                 engine_factory=None, comm=None, ipc=None, strict=False, snapshot=None, policy=None, txlog=False,
                 course=False, disease=None, defer_ipc=False):
    """Build a Context the way calc/simulation.py:148-180 does.  `disease` (engine.Disease): a ready disease block the
    engine is created with, in place of the one built from the variables (parameters.expand_numpy).  `defer_ipc`: the initial
    population condition is not applied yet; Context.apply_initial_condition() applies it (it draws from the disease block:
    ensemble.run_parameter_ensemble sets the member's block first).  `ipc`: an InitialPopulationCondition,
    a dict of its fields, None (no initial condition), or 'auto' = what simulate_individuals passes,
    datasets.get_initial_population_condition(variables) (calc/simulation.py:152).
    `snapshot` (snapshot.Snapshot): the Context continues from it (Context.restore); no initial condition is applied, the
    state is replaced.  `policy` (policy.Policy): triggered interventions -- run() takes the policy route.
    `txlog`: keep a dated transmission log (Context.start_transmission_log; begun after the restore when a snapshot is given:
    everything the snapshot holds is BEFORE).  `course`: keep a clinical course log as well (Context.start_course_log); implies
    `txlog`."""
    if snapshot is not None:
        ipc = None
    if isinstance(ipc, str) and ipc == 'auto':
        ipc = datasets.get_initial_population_condition(variables)
    if age_counts is None:
        age_counts = datasets.get_population_for_area(variables['area_name'])
    age_to_group = datasets.make_age_groups(variables['max_age'])
    groups = list(np.unique(age_to_group))
    pop_params = dict(
        age_structure=np.asarray(age_counts),
        contacts_per_day=datasets.get_contacts_per_day(variables['country']),
        initial_population_condition=datasets.InitialPopulationCondition(**ipc) if isinstance(ipc, dict) else ipc,
        defer_initial_population_condition=bool(defer_ipc),
        age_groups=dict(labels=groups, age_indices=[groups.index(x) for x in age_to_group]),
        imported_infection_ages=variables['imported_infection_ages'],
    )
    hc = dict(hospital_beds=variables['hospital_beds'], icu_units=variables['icu_units'])
    ctx = model.Context(pop_params, hc, create_disease_params(variables), variables['start_date'],
                        random_seed=variables['random_seed'] if seed is None else seed,
                        device=device, engine_factory=engine_factory, comm=comm, strict=strict, policy=policy,
                        txlog=bool(txlog) and snapshot is None, course=bool(course) and snapshot is None, disease=disease)
    if interventions is None:
        ivs = get_active_interventions(variables)
    else:
        vnames = tuple(v['name'] for v in variables['variants'])
        ivs = [iv_tuple_to_obj(iv, vnames) for iv in interventions]
    for iv in ivs:
        ctx.add_intervention(iv)
    if snapshot is not None:
        ctx.restore(snapshot)
        if txlog or course:
            ctx.start_transmission_log()
        if course:
            ctx.start_course_log()
    return ctx


def simulate_individuals(variables=None, step_callback=None, callback_day_interval=1, device='cuda:0',
                         engine_factory=None, age_counts=None, policy=None):
    """`policy` (policy.Policy): the run reacts to its own counters; df's mobility_limitation follows the levels and df gets a
    `policy_level` column (the level in force on each date)."""
    import pandas as pd
    if variables is None:
        variables = copy_variables()
    t0 = time.perf_counter()
    ctx = make_context(variables, age_counts=age_counts, device=device, engine_factory=engine_factory,
                       ipc=datasets.get_initial_population_condition(variables), policy=policy)   # calc/simulation.py:152
    start_date = date.fromisoformat(variables['start_date'])
    days = variables['simulation_days']
    age_groups = ctx.age_group_labels
    date_index = pd.date_range(start_date, periods=days)
    cols = POP_ATTRS + STATE_ATTRS + EXPOSURES_ATTRS + ['us_per_infected']
    rows = []
    ag_array = np.empty((days, len(POP_ATTRS), len(age_groups)), dtype='i')

    if step_callback is None:   # no progress reports wanted: one run, frames for all days at once
        last = time.perf_counter()
        hist = ctx.run(days)
        df, adf = _frames_from_history(ctx, hist, ctx.mobility_history, start_date, (time.perf_counter() - last) * 1000 / days)
        if policy is not None:
            df['policy_level'] = np.asarray(ctx.policy_levels, dtype=np.int64)
        return df, adf

    done = 0
    stretch = max(1, int(callback_day_interval))
    last = time.perf_counter()
    levels = []
    while done < days:
        n = min(stretch, days - done)
        hist = ctx.run(n)
        if policy is not None:
            levels += [int(x) for x in ctx.policy_levels]
        now = time.perf_counter()
        ms_per_day = (now - last) * 1000 / n
        last = now
        for k in range(n):
            s = ctx.state_from_counters(hist[k], mobility_factor=ctx.mobility_history[k])
            for idx, attr in enumerate(POP_ATTRS):
                ag_array[done + k, idx, :] = s[attr]
            rec = {attr: s[attr].sum() for attr in POP_ATTRS}
            for a in STATE_ATTRS:
                rec[a] = s[a]
            for place, nr in s['daily_contacts'].items():
                rec['exposures_%s' % place] = nr
            rec['us_per_infected'] = ms_per_day * 1000 / rec['infected'] if rec['infected'] else 0
            rows.append(rec)
        done += n
        df = pd.DataFrame(rows, index=date_index[:done], columns=cols).reindex(date_index)
        if not step_callback(df):
            raise ExecutionInterrupted()
    df = pd.DataFrame(rows, index=date_index, columns=cols).astype(np.float64).astype(object)
    if policy is not None:
        df['policy_level'] = np.asarray(levels, dtype=np.int64)
    adf = pd.DataFrame(
        ag_array.flatten(),
        index=pd.MultiIndex.from_product([date_index, POP_ATTRS, age_groups], names=['date', 'attr', 'age_group']),
        columns=['pop'])
    adf = adf.unstack('attr').unstack('age_group')
    adf.columns = adf.columns.droplevel()
    return df, adf


def simulate_with_snapshots(variables=None, snapshot_days=(), days=None, device='cuda:0', engine_factory=None, age_counts=None):
    """simulate_individuals' run that also takes a snapshot (snapshot.Snapshot) before each of `snapshot_days` (0 <= d <=
    days).  Returns (df, adf, {day: Snapshot}); each snapshot carries the history rows and mobility history of the days
    before it, so resume_individuals can give the frames of the whole horizon."""
    if variables is None:
        variables = copy_variables()
    ctx = make_context(variables, age_counts=age_counts, device=device, engine_factory=engine_factory,
                       ipc=datasets.get_initial_population_condition(variables))
    days = variables['simulation_days'] if days is None else int(days)
    wanted = sorted(set(int(d) for d in snapshot_days))
    if wanted and (wanted[0] < 0 or wanted[-1] > days):
        raise ValueError('snapshot days must lie in [0, %d]' % days)
    t0 = time.perf_counter()
    hists, mobility, snaps, done = [], [], {}, 0
    for d in wanted + [days]:
        if d > done:
            hists.append(ctx.run(d - done))
            mobility += ctx.mobility_history
            done = d
        if d in wanted:
            h = np.concatenate(hists) if hists else np.zeros((0, _eng.COUNTER_WORDS), dtype=np.int32)
            snaps[d] = ctx.snapshot().with_history(h, list(mobility))
    hist = np.concatenate(hists) if hists else np.zeros((0, _eng.COUNTER_WORDS), dtype=np.int32)
    df, adf = _frames_from_history(ctx, hist, mobility, date.fromisoformat(variables['start_date']),
                                   (time.perf_counter() - t0) * 1000 / max(days, 1))
    return df, adf, snaps


def resume_individuals(snap, variables=None, seed=None, device='cuda:0', engine_factory=None, age_counts=None):
    """simulate_individuals' frames for the whole horizon of `variables`, the days before `snap` from its history and the rest
    run from it -- with `variables`' own interventions from the snapshot's day on (a what-if of the future), and `seed` (default:
    the snapshot's) for the days to come."""
    if variables is None:
        variables = copy_variables()
    if snap.history is None:
        raise ValueError('resume_individuals: the snapshot carries no history (take it with simulate_with_snapshots)')
    ctx = make_context(variables, age_counts=age_counts, seed=snap.seed if seed is None else seed, device=device,
                       engine_factory=engine_factory, snapshot=snap)
    days = variables['simulation_days']
    t0 = time.perf_counter()
    rest = ctx.run(days - snap.day) if days > snap.day else np.zeros((0, _eng.COUNTER_WORDS), dtype=np.int32)
    ms = (time.perf_counter() - t0) * 1000 / max(days - snap.day, 1)
    hist = np.concatenate([snap.history, rest])
    mobility = list(snap.mobility_history) + list(ctx.mobility_history if days > snap.day else [])
    return _frames_from_history(ctx, hist, mobility, date.fromisoformat(variables['start_date']), ms)


def _frames_from_history(ctx, hist, mobility_history, start_date, ms_per_day=0.0, want_adf=True):
    """(df, adf) of simulate_individuals from a recorded counter history[days, COUNTER_WORDS]; all
    days at once (the per-day dict path, Context.state_from_counters, gives the same numbers -- checked
    in tests/test_host_logic.py)."""
    import pandas as pd
    days = hist.shape[0]
    A = _eng.MAX_AGES
    age_groups = ctx.age_group_labels
    ngroups = len(age_groups)
    date_index = pd.date_range(start_date, periods=days)
    cols = POP_ATTRS + STATE_ATTRS + EXPOSURES_ATTRS + ['us_per_infected']
    # age -> report group sums as one matrix product per attribute: [days, nr_ages] @ [nr_ages, groups]
    onehot = np.zeros((ctx.nr_ages, ngroups), dtype=np.int64)
    onehot[np.arange(ctx.nr_ages), ctx.age_group_indices[:ctx.nr_ages]] = 1
    ag_array = np.empty((days, len(POP_ATTRS), ngroups), dtype='i')
    data = {}
    for idx, attr in enumerate(POP_ATTRS):
        ci = _eng.C_NAMES.index(attr)
        per_age = hist[:, ci * A: ci * A + ctx.nr_ages].astype(np.int64)
        ag_array[:, idx, :] = per_age @ onehot
        data[attr] = ag_array[:, idx, :].sum(axis=1)
    sc = hist[:, _eng.C_NR * A:].astype(np.int64)
    infections, infectors = sc[:, _eng.S_TOTAL_INFECTIONS], sc[:, _eng.S_TOTAL_INFECTORS]
    r = np.zeros(days, dtype=np.float64)   # 0 until more than 5 infectors were seen (main.pyx:1827)
    ok = infectors > 5
    r[ok] = infections[ok] / infectors[ok]
    data['exposed_per_day'] = sc[:, _eng.S_EXPOSED_PER_DAY]
    data['available_hospital_beds'] = sc[:, _eng.S_AVAILABLE_BEDS]
    data['available_icu_units'] = sc[:, _eng.S_AVAILABLE_ICU]
    data['total_icu_units'] = sc[:, _eng.S_ICU_UNITS]
    data['ct_cases_per_day'] = sc[:, _eng.S_CT_CASES_PER_DAY]
    data['r'] = r
    data['mobility_limitation'] = 1 - np.asarray(mobility_history[:days], dtype=np.float64)
    for i, place in enumerate(model.PLACES):
        data['exposures_%s' % place] = sc[:, _eng.S_DAILY_CONTACTS + i]
    infected = data['infected'].astype(np.float64)
    data['us_per_infected'] = np.where(infected > 0, ms_per_day * 1000 / np.where(infected > 0, infected, 1), 0)
    # (the reference assembles its frame from per-day dicts and reindexes it on every progress report: what reaches the caller
    # holds Python floats in object columns -- recorded from the real driver in tests/golden/frames_ref.json; same here)
    df = pd.DataFrame({c: np.asarray(data[c], dtype=np.float64) for c in cols}, index=date_index, columns=cols).astype(object)
    if not want_adf:
        return df, None
    adf = pd.DataFrame(
        ag_array.flatten(),
        index=pd.MultiIndex.from_product([date_index, POP_ATTRS, age_groups], names=['date', 'attr', 'age_group']),
        columns=['pop'])
    adf = adf.unstack('attr').unstack('age_group')
    adf.columns = adf.columns.droplevel()
    return df, adf


def sample_model_parameters(what, age, severity=None, variables=None, device='cuda:0', engine_factory=None):
    """calc/simulation.py:301-347: distribution of one per-agent quantity (`Context.sample`) in a
    one-agent-per-age population.  Returns the value -> share Series (severity names for
    'symptom_severity'; the day -> infectiousness Series for 'infectiousness').  The reference
    also prints the table and opens a matplotlib window; that is left to the caller."""
    import pandas as pd
    if variables is None:
        variables = copy_variables()
    max_age = variables['max_age']
    age_to_group = datasets.make_age_groups(max_age)
    groups = list(np.unique(age_to_group))
    pop_params = dict(
        age_structure=np.ones(max_age + 1, dtype=np.int64),
        contacts_per_day=datasets.get_contacts_per_day(variables['country']),
        age_groups=dict(labels=groups, age_indices=[groups.index(x) for x in age_to_group]),
        imported_infection_ages=variables['imported_infection_ages'],   # (the reference omits it and fails)
    )
    ctx = model.Context(pop_params, dict(hospital_beds=0, icu_units=0), create_disease_params(variables),
                        '2020-01-01', device=device, engine_factory=engine_factory)
    if variables.get('sample_limit_mobility', 0) != 0:
        # the reference passes (type, value) to apply_intervention, which only accepts an
        # intervention object (main.pyx:1880); the evident intent is a population-wide limit
        ctx.apply_intervention(iv_tuple_to_obj(['limit-mobility', None, variables['sample_limit_mobility']],
                                               tuple(v['name'] for v in variables['variants'])))
        ctx.contact_matrix.init_day()
    samples = ctx.sample(what, age, severity)
    if what == 'infectiousness':
        s = pd.Series(index=samples['day'], data=samples['val'])
        return s[s != 0].sort_index()
    s = pd.Series(samples)
    c = s.value_counts().sort_index()
    if what == 'symptom_severity':
        c.index = c.index.map(model.SEVERITY_TO_STR)
    return c / c.sum()


def simulate_monte_carlo(seed, variables=None, device='cuda:0', engine_factory=None, age_counts=None):
    """calc/simulation.py:350-359: one run with `random_seed = seed`; df gets a 'run' column."""
    v = copy_variables() if variables is None else dict(variables)
    v['random_seed'] = seed
    df, _ = simulate_individuals(v, device=device, engine_factory=engine_factory, age_counts=age_counts)
    df['run'] = seed
    return df


def run_monte_carlo(scenario_name, seeds=range(1000), device='cuda:0', group_size=64, days=None, write_csv=True,
                    age_counts=None, engine_factory=None, variables=None, ipc='auto', summary=None):
    """calc/simulation.py:362-385 with the seeds stepped as engine groups on one GPU instead of a
    process pool: one DataFrame with every run's per-date rows, columns as simulate_individuals
    plus 'run' and 'scenario'; written to reina_<scenario>.csv like the reference.  Every run starts from
    the scenario's initial population condition, as the reference's do (run_monte_carlo ->
    simulate_monte_carlo -> simulate_individuals, calc/simulation.py:152); `ipc` overrides it.
    `summary` (summary.SummarySpec): the EnsembleSummary of all seeds instead of the frame (quantile bands, peaks, exceedance:
    reina_model_amd/summary.py) -- no history is read back, no frame per run is built; with write_csv its frame() goes to
    reina_<scenario>_bands.csv."""
    import pandas as pd
    from . import ensemble
    from .scenarios import scenario_variables
    v = scenario_variables(scenario_name, base=variables)
    days = v['simulation_days'] if days is None else days
    seeds = list(seeds)
    dfs = []
    # (ensemble.Setup / plan_once: ONE planner and one plan for all chunks -- the plan does not depend on the seed)
    setup = ensemble.Setup(age_counts, device, engine_factory, None, ipc)
    plan, pending = ensemble.plan_once(setup, v, seeds[0], days, summary)
    for part in ensemble.chunks(seeds, group_size):
        members = setup.members(v, part)
        t0 = time.perf_counter()
        hist = ensemble.run_group_plan(members, plan, summary=pending)
        ms_per_day = (time.perf_counter() - t0) * 1000 / days / len(part)
        for m, sd in enumerate(part if summary is None else ()):
            df, _ = _frames_from_history(members[m], hist[m], plan['mobility_history'],
                                         date.fromisoformat(v['start_date']), ms_per_day, want_adf=False)
            df['run'] = sd
            dfs.append(df)
        del members
    if summary is not None:
        out = pending.finish(members=seeds)
        if write_csv:
            out.frame().to_csv('reina_%s_bands.csv' % scenario_name)
        return out
    df = pd.concat(dfs)
    df.index.name = 'date'
    df = df.reset_index()
    df['scenario'] = scenario_name
    if write_csv:
        df.to_csv('reina_%s.csv' % scenario_name, index=False)
    return df


def table_header():
    """header line of the day table the reference prints when run as a script (calc/simulation.py:411-421)"""
    header = '%-10s' % 'day'
    for attr in POP_ATTRS + ['ct_cases_per_day', 'r'] + ['exposures', 'us_per_infected']:
        header += '%15s' % attr
    return header


def table_row(rec):
    """one line of that table from a row of df (calc/simulation.py:423-441)"""
    s = '%-12s' % rec.name.date().isoformat()
    for attr in POP_ATTRS:
        s += '%15d' % rec[attr]
    s += '%15d' % rec['ct_cases_per_day']
    s += '%13.2f' % rec['r']
    s += '%15d' % sum(rec[x] for x in rec.index if 'exposures_' in x)
    if rec['infected']:
        s += '%13.2f' % rec['us_per_infected']
    return s


def main(argv=None):
    """The day table the reference prints when run as a script (calc/simulation.py:411-447)."""
    import argparse
    from .scenarios import scenario_variables
    ap = argparse.ArgumentParser(prog='python -m reina_model_amd.simulation')
    ap.add_argument('--days', type=int, default=None)
    ap.add_argument('--seed', type=int, default=None)
    ap.add_argument('--scenario', default='default')
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--interval', type=int, default=1, help='days between printed rows')
    a = ap.parse_args(argv)
    v = scenario_variables(a.scenario)
    if a.days is not None:
        v['simulation_days'] = a.days
    if a.seed is not None:
        v['random_seed'] = a.seed
    print(table_header())

    def step_callback(df):
        for _, rec in df.dropna().iloc[-a.interval:].iterrows():
            print(table_row(rec))
        return True

    df, adf = simulate_individuals(v, step_callback=step_callback, callback_day_interval=a.interval, device=a.device)
    print(adf)
    return df, adf


if __name__ == '__main__':
    main()
