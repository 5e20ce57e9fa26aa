"""Test-side definitions of the ensemble-route tests: the scenario, the routes and what is kept of a route's result, in ONE
place.  tests/test_ensemble_routes.py holds them to a recording on oracle B; tests/test_ensemble_routes_gpu.py runs them on
the device against oracle B."""
import contextlib
import functools
import zlib

import numpy as np

import filter_util
from reina_model_amd import engine as eng, ensemble, filtering, model, policy as pol, simulation, summary as sm

SEEDS = [11, 12, 13]
DAYS = 12
SNAP_DAY = 5
WINDOW = 6
FORECAST = 3
TRUTH_SEED = 901


@functools.lru_cache(maxsize=None)
def scenario(value=None, when='2020-02-26'):
    """(variables, ages) of filter_util.small_scenario(20000); with `value`, a population-wide mobility limit from `when` on
    (2020-02-26 is day 8)"""
    v, ages = filter_util.small_scenario(20000)
    if value is not None:
        v['interventions'] = [list(iv) for iv in v['interventions']] + [['limit-mobility', when, value]]
    return v, ages


def the_policy():
    """people infected, reviewed daily: the three seeds reach level 1 on days 9, 10 and 7"""
    return pol.Policy(pol.Signal('infected'), levels=[[], [['limit-mobility', 40]], [['limit-mobility', 60], ['wear-masks', 50]]],
                      up=[40, 60], down=[10, 30], review_every=1, min_days=2)


def the_spec():
    return sm.SummarySpec(quantiles=(0.0, 0.5, 1.0), thresholds=(('infected', 30), ('all_detected', 5)))


def _kw(factory):
    return dict(age_counts=scenario()[1], engine_factory=factory)


@functools.lru_cache(maxsize=None)
def snapshot(factory):
    v, ages = scenario()
    c = simulation.make_context(v, ipc='auto', seed=SEEDS[0], **_kw(factory))
    c.run(SNAP_DAY)
    return c.snapshot()


@functools.lru_cache(maxsize=None)
def truth():
    """the history the filter's observations are taken of: oracle B's, whatever engines the filter runs on"""
    import par_backend
    v, ages = scenario()
    return simulation.make_context(v, ipc='auto', seed=TRUTH_SEED, **_kw(par_backend.par_engine_factory)).run(SNAP_DAY + DAYS)


def _filter(factory, snap):
    v, ages = scenario()
    first = SNAP_DAY if snap else 0
    # (the dates of ONE window only -- the second from day 0, where the first sees no case yet; the first from the snapshot --
    # so that the members are resampled once)
    rows = range(first + 1, first + WINDOW) if snap else range(WINDOW + 1, 2 * WINDOW)
    obs = filter_util.observations(truth(), v['start_date'], rows, streams=('all_detected',))
    res = filtering.particle_filter(v, len(SEEDS), observations=obs, obs_model=filtering.ObservationModel({'all_detected': 50.0}),
                                    window=WINDOW, days=DAYS, seeds=SEEDS, filter_seed=4, ess_threshold=0.99,
                                    snapshot=snapshot(factory) if snap else None, **_kw(factory))
    return res


def _monte_carlo(factory, **kw):
    v, ages = scenario()
    return simulation.run_monte_carlo('default', seeds=SEEDS, days=DAYS, group_size=2, write_csv=False, variables=v,
                                      **_kw(factory), **kw)


def _foreign(factory, call):
    """`call` on two Contexts with the group of two others"""
    v, ages = scenario()
    mk = lambda sd: simulation.make_context(v, ipc='auto', seed=sd, **_kw(factory))
    ctxs, others = [mk(1), mk(2)], [mk(3), mk(4)]
    group = eng.EngineGroup([c.engine for c in others])
    try:
        return call(ctxs, mk(1), group)
    finally:
        group.close()


def _routes(factory):
    v, ages = scenario()
    kw = _kw(factory)
    sweep = lambda vs: ensemble.run_sweep(vs, SEEDS, DAYS, **kw)
    branches = lambda **more: ensemble.run_branches(snapshot(factory), v, SEEDS, DAYS, **kw, **more)
    three = [scenario(10)[0], scenario(30)[0], scenario(50)[0]]
    return dict(
        ensemble=lambda: ensemble.run_ensemble(v, SEEDS, DAYS, concurrent=2, **kw),
        ensemble_summary=lambda: ensemble.run_ensemble(v, SEEDS, DAYS, concurrent=2, summary=the_spec(), **kw),
        sweep=lambda: sweep(three),
        sweep_date=lambda: sweep([three[0], three[1], scenario(50, '2020-02-27')[0]]),
        policy_ensemble=lambda: ensemble.run_policy_ensemble(v, SEEDS, DAYS, the_policy(), **kw),
        branches=branches,
        branches_members=lambda: branches(member_variables=three),
        branches_policy=lambda: branches(policy=the_policy()),
        branches_policy_members=lambda: branches(member_variables=three, policy=the_policy()),
        filter=lambda: _filter(factory, False),
        filter_snapshot=lambda: _filter(factory, True),
        monte_carlo=lambda: _monte_carlo(factory),
        monte_carlo_summary=lambda: _monte_carlo(factory, summary=the_spec()),
        foreign_group_plan=lambda: _foreign(factory, lambda ctxs, planner, g: ensemble.run_group_plan(ctxs, planner.make_plan(DAYS), group=g)),
        foreign_group_reports=lambda: _foreign(factory, lambda ctxs, planner, g: ensemble.transmission_reports(ctxs, group=g)),
    )


CASES = tuple(_routes(None))


def run(name, factory):
    """the route's own return value (factory: an engine factory, None for the HIP engine)"""
    return _routes(factory)[name]()


# ------------------------------------------------------------------------------------------------ what a route built

class Built:
    """Counts, while it is entered, the calls of simulation.make_context (keeping the Contexts), of Context.make_plan (a
    Context that makes a plan is a planner, every other one a member), of EngineGroup.__init__ and of the close of an open
    group."""

    def __enter__(self):
        self.contexts, self.planners, self.groups, self.closed = [], set(), 0, 0
        self._saved = (simulation.make_context, model.Context.make_plan, eng.EngineGroup.__init__)
        make_context, make_plan, init = self._saved

        def counted_context(*a, **kw):
            c = make_context(*a, **kw)
            self.contexts.append(c)
            return c

        def counted_plan(ctx, *a, **kw):
            self.planners.add(id(ctx))
            return make_plan(ctx, *a, **kw)

        def counted_init(group, *a, **kw):
            init(group, *a, **kw)
            self.groups += 1

        def counted_close(group):
            self.closed += bool(group._h)
            eng.Handle.close(group)

        simulation.make_context, model.Context.make_plan = counted_context, counted_plan
        eng.EngineGroup.__init__, eng.EngineGroup.close = counted_init, counted_close
        return self

    def __exit__(self, *exc):
        simulation.make_context, model.Context.make_plan, eng.EngineGroup.__init__ = self._saved
        del eng.EngineGroup.close

    def members(self):
        return [c for c in self.contexts if id(c) not in self.planners]

    def counts(self):
        return dict(planners=len(self.planners), members=len(self.contexts) - len(self.planners), groups=self.groups,
                    open=self.groups - self.closed)


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def _member(c):
    out = dict(day=int(c.day), mobility_history=[float(x) for x in getattr(c, 'mobility_history', ())])   # (none: it ran no day)
    if getattr(c, 'policy_levels', None) is not None:
        out['policy_levels'] = [int(x) for x in c.policy_levels]
    return out


def frame_values(df):
    """the frame of run_monte_carlo as float64, without the column that is a wall time"""
    return df.drop(columns=['date', 'scenario', 'us_per_infected']).to_numpy(dtype=np.float64)


def result(r):
    """what is compared of a route's return value: a history, a summary's words or a frame's values"""
    import pandas as pd
    if isinstance(r, tuple):
        r = r[0]
    if isinstance(r, filtering.FilterResult):
        return r.paths()
    if isinstance(r, sm.EnsembleSummary):
        return r.words
    if isinstance(r, pd.DataFrame):
        return frame_values(r)
    return np.asarray(r)


def record(name, factory):
    """The case `name` as JSON: the crc32 of result(), the members, what was built -- or the refusal's type and text"""
    snapshot(factory), truth()        # (made once, ahead of the count)
    with Built() as built:
        out = {}
        try:
            r = run(name, factory)
        except Exception as e:        # noqa: BLE001  (the refusals are cases too)
            out['error'] = [type(e).__name__, str(e)]
        else:
            if name.startswith('foreign'):     # (host-memory engines take no group for their reports: nothing is refused)
                out['returned'] = type(r).__name__
            else:
                out['crc'], out['shape'] = crc(result(r)), list(result(r).shape)
            if isinstance(r, tuple) and len(r) == 3:
                out['levels'] = crc(np.asarray(r[1], dtype=np.int32))
            if isinstance(r, filtering.FilterResult):
                out.update(log_evidence=float(r.log_evidence), ancestors=[[int(x) for x in w['ancestors']] for w in r.windows],
                           ess=[float(w['ess']) for w in r.windows], resampled=[bool(w['resampled']) for w in r.windows],
                           pairs=[int(t['pairs']) for t in r.timings])
        out['built'] = built.counts()
        if not name.startswith('foreign'):
            out['members'] = [_member(c) for c in built.members()]
        if 'error' not in out and isinstance(r, filtering.FilterResult):
            fc = r.forecast(FORECAST)
            out.update(forecast=crc(fc), members_after_forecast=[_member(c) for c in r.contexts], open_after_forecast=built.counts()['open'])
            r.close()
            out['open_after_close'] = built.counts()['open']
    return out


@contextlib.contextmanager
def closing(r):
    """a route's return value; a filter's group is closed on the way out"""
    try:
        yield r
    finally:
        if isinstance(r, filtering.FilterResult):
            r.close()
