"""The routes of tests/test_ensemble_routes.py on the device: every route's result on the HIP engine equals the same route on
oracle B engines run in the same test (ensemble_routes_util.py holds the routes: the same scenario, members and days), a foreign
`group` is refused with each route's own words, and the threaded run_ensemble, which has no CPU form, equals the batched one."""
import numpy as np
import pytest

import ensemble_routes_util as ru
import par_backend
import policy_util as pu
from reina_model_amd import engine as eng, ensemble, policy as pol

pytestmark = pytest.mark.gpu
PAR = par_backend.par_engine_factory

# (branches_policy: oracle B has no device route to compare with -- test_branches_under_a_policy; the refusals: below)
SAME = tuple(n for n in ru.CASES if n not in ('sweep_date', 'branches_policy', 'branches_policy_members', 'foreign_group_plan',
                                              'foreign_group_reports'))


def _members(r):
    return r.contexts if hasattr(r, 'contexts') else r[-1] if isinstance(r, tuple) else ()


@pytest.mark.parametrize('name', SAME)
def test_route_on_the_device_equals_the_route_on_oracle_b(name):
    with ru.closing(ru.run(name, None)) as dev, ru.closing(ru.run(name, PAR)) as cpu:
        got, want = ru.result(dev), ru.result(cpu)
        assert got.shape == want.shape and np.array_equal(got, want)
        assert len(_members(dev)) == len(_members(cpu))
        for m, (a, b) in enumerate(zip(_members(dev), _members(cpu))):
            assert eng.is_device(a.engine) and not eng.is_device(b.engine)
            assert a.day == b.day and list(a.mobility_history) == list(b.mobility_history), m
            assert np.array_equal(a.engine.read_counters(), b.engine.read_counters()), 'member %d' % m
        if name == 'policy_ensemble':      # (the device route against the host-driven fallback)
            assert dev[2][0].engine.policy_f is not None and cpu[2][0].engine.policy_f is None
            assert np.array_equal(dev[1], cpu[1]) and len({tuple(lv) for lv in dev[1]}) == len(ru.SEEDS)
        if name.startswith('filter'):
            assert dev.log_evidence == cpu.log_evidence and np.array_equal(dev.ancestors, cpu.ancestors)
            assert np.array_equal(dev.ess, cpu.ess) and any(t['pairs'] for t in dev.timings)
            assert np.array_equal(dev.forecast(ru.FORECAST), cpu.forecast(ru.FORECAST))


def test_branches_under_a_policy():
    """every future of the snapshot under the policy on the device == oracle B restored from the same snapshot with the member's
    seed, driven from the host"""
    snap, (v, ages) = ru.snapshot(None), ru.scenario()
    hist, ctxs = ru.run('branches_policy', None)
    for m, sd in enumerate(ru.SEEDS):
        ref = pu.make(v, ages, seed=sd, factory=PAR, snapshot=snap, ipc=None)
        assert np.array_equal(hist[m], pol.run_host_driven(ref, ru.the_policy(), ru.DAYS)), m
        assert np.array_equal(ctxs[m].policy_levels, ref.policy_levels), m
    assert len({tuple(c.policy_levels) for c in ctxs}) > 1


@pytest.mark.parametrize('name,words', [
    ('sweep_date', 'scenario 2 differs from scenario 0 in more than the values of its mobility / mask interventions: it cannot share a group'),
    ('branches_policy_members', 'run_branches: a policy and member_variables cannot be combined'),
    ('foreign_group_plan', 'run_group_plan: `group` is not the group of these contexts'),
    ('foreign_group_reports', 'transmission_reports: `group` is not the group of these contexts')])
def test_refusals_on_the_device(name, words):
    with pytest.raises(ValueError) as e:
        ru.run(name, None)
    assert str(e.value) == words


def test_threaded_run_ensemble_equals_batched():
    v, ages = ru.scenario()
    batched = ru.run('ensemble', None)
    threaded = ensemble.run_ensemble(v, ru.SEEDS, ru.DAYS, age_counts=ages, batched=False, concurrent=2, threads=2)
    assert np.array_equal(batched, threaded)
    a = ensemble.run_ensemble(v, ru.SEEDS, ru.DAYS, age_counts=ages, batched=False, summary=ru.the_spec())
    assert np.array_equal(a.words, ru.run('ensemble_summary', None).words)
