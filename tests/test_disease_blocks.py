"""The case table of tests/disease_block_util.py held honest without a GPU: every case runs on oracle B and is a real epidemic
(the floors below keep a case of tests/test_disease_blocks_gpu.py from passing on an empty one), the failing cases fail on the
recorded iterate() with the recorded text, and every block differs from the base in exactly the fields its knobs name."""
import ctypes

import numpy as np
import pytest

import disease_block_util as dbu
import filter_util
import par_backend
from reina_model_amd import engine as eng
from reina_model_amd import ensemble, simulation
from reina_model_amd import parameters as par
from reina_model_amd.model import SimulationFailed
from reina_model_amd.parameters import ParameterSpace

PAR = par_backend.par_engine_factory
PROBLEM = eng.C_NR * eng.MAX_AGES + eng.S_PROBLEM


def _context(case, **kw):
    v, ages = dbu.scenario()
    return simulation.make_context(v, age_counts=ages, seed=dbu.SEED, ipc='auto', interventions=dbu.interventions_of(case, v),
                                   engine_factory=PAR, disease=dbu.block_of(case), **kw)


def _field_bytes(d, name):
    x = getattr(d, name)
    return ctypes.string_at(x, ctypes.sizeof(x)) if hasattr(x, '__len__') else x


@pytest.mark.parametrize('case', dbu.CASES + dbu.FAILING + [dbu.SHARDED], ids=lambda c: c.name)
def test_a_block_differs_from_the_base_in_the_named_fields_only(case):
    """(tests/test_params.py: _same_outside)  Every field no knob names is the base's byte for byte; inside a named field every
    word outside the knob's cells (variants, ages) is the base's; and every knob moves its cells -- but a probability that the
    base already holds at 1 everywhere and a theta >= 1 would clamp back to it (p_icu_death_no_beds of the bundled block)."""
    base, block = dbu.base_block(), dbu.block_of(case)
    for name, _ in eng.Disease._fields_:
        if name not in case.fields:
            assert _field_bytes(block, name) == _field_bytes(base, name), name
    words = lambda d: np.frombuffer(par.disease_bytes(d), dtype=np.uint32)
    wb, wd = words(base), words(block)
    covered = np.zeros(len(wb), dtype=bool)
    for (f, mask, lo, hi), theta in zip(case.space.table(dbu.A, dbu.V), case.theta):
        name = par.FIELDS[f]
        w0 = getattr(eng.Disease, name).offset // 4
        if name in par.SCALAR_FIELDS:
            idx = [w0 + v for v in range(eng.MAX_VARIANTS) if mask >> v & 1]
        elif name in par.AGE_FIELDS:
            idx = list(range(w0 + lo, w0 + hi + 1))
        else:
            idx = [w0 + v * eng.MAX_AGES + a for v in range(eng.MAX_VARIANTS) if mask >> v & 1 for a in range(lo, hi + 1)]
        assert not covered[idx].any()
        covered[idx] = True
        held_at_one = name in par.CLAMPED and theta >= 1 and np.all(wb[idx].view(np.float32) == 1)
        assert np.any(wd[idx] != wb[idx]) == (not held_at_one), name
    assert not np.any((wd != wb) & ~covered)
    assert np.any(wd != wb)


@pytest.mark.parametrize('case', dbu.CASES, ids=dbu.CASE_NAMES)
def test_a_case_is_an_epidemic_on_oracle_b(case):
    ctx = _context(case)
    hist = ctx.run(dbu.DAYS)
    got = dbu.ends(hist)
    print(case.name, got)
    assert not hist[:, PROBLEM].any()
    assert got == case.recorded
    assert got[0] >= dbu.MIN_INFECTED
    if case.deaths:
        assert got[1] >= dbu.MIN_DEAD
    if case.variant1:
        assert dbu.carries_variant1(ctx) >= dbu.MIN_VARIANT1
    if 'p_death_outside_hospital' in case.fields:   # (severity_of's outside-hospital branch is the one that runs)
        assert filter_util.totals(hist, 'non_hospital_deaths')[-1] >= dbu.MIN_DEAD
    if case.strict_days:   # a case close under a failing one: it must NOT fail
        ctx = _context(case, strict=True)
        for _ in range(case.strict_days):
            ctx.iterate()


def test_the_floors_cover_the_cases_they_are_meant_for():
    """every case that scales a severity or death field holds the deaths floor, but the two whose recorded ends are 0 and 2 dead"""
    deadly = set(par.AGE_FIELDS) | {'p_hospital_death_no_beds', 'p_icu_death_no_beds', 'mean_duration_from_onset_to_death'}
    for case in dbu.CASES:
        if case.name in ('nobody symptomatic', 'no transmission'):
            assert not case.deaths
        else:
            assert case.deaths == bool(deadly & set(case.fields)), case.name
    assert len(dbu.CASES) == 13 and len(set(dbu.CASE_NAMES)) == 13


@pytest.mark.parametrize('case', dbu.FAILING, ids=dbu.FAILING_NAMES)
def test_a_failing_case_fails_on_the_recorded_day(case):
    ctx = _context(case, strict=True)
    assert case.recorded >= 1
    for _ in range(case.recorded):
        ctx.iterate()
    with pytest.raises(SimulationFailed) as ei:
        ctx.iterate()
    assert str(ei.value) == dbu.FAIL_TEXT


@pytest.mark.parametrize('attribution', ['exact', 'mirror'])
def test_the_sharded_case_is_an_epidemic_on_oracle_b(attribution):
    from reina_model_amd import sharding
    v, ages = dbu.scenario()
    members = []
    cpu = [simulation.make_context(v, age_counts=ages, seed=dbu.SHARDED_SEED, ipc='auto', engine_factory=PAR, disease=dbu.block_of(dbu.SHARDED),
                                   comm=sharding.InProcessComm(r, 2, members, attribution=attribution)) for r in range(2)]
    for _ in range(dbu.DAYS):
        sharding.step_shards_together(cpu)
    tot = sharding.reduce_counters(cpu)
    infected = int(tot[eng.C_NAMES.index('all_infected') * eng.MAX_AGES:][:eng.MAX_AGES].sum())
    print(attribution, infected)
    assert not tot[PROBLEM]
    assert infected == dbu.SHARDED.recorded[attribution] and infected >= dbu.SHARDED_MIN_INFECTED


@pytest.mark.parametrize('name', ['A', 'B'])
def test_the_group_spaces_run_on_oracle_b_and_no_member_fails(name):
    space = ParameterSpace(dbu.GROUP_SPACES[name])
    v, ages = dbu.scenario()
    thetas = dbu.group_thetas()
    assert thetas.shape == (6, 8) and np.all(thetas[0] == 1) and thetas[1:].min() >= np.float32(0.4) and thetas[1:].max() <= np.float32(2.0)
    hist, ctxs = ensemble.run_parameter_ensemble(v, thetas, dbu.GROUP_SEEDS, dbu.DAYS, space, age_counts=ages, engine_factory=PAR)
    assert hist.shape == (6, dbu.DAYS, eng.COUNTER_WORDS)
    assert not hist[:, :, PROBLEM].any()
    infected = filter_util.totals(hist, 'all_infected')[:, -1]
    print(name, infected.tolist())
    assert infected.tolist() == dbu.GROUP_RECORDED[name]
    assert infected.min() >= dbu.GROUP_MIN_INFECTED and len(set(infected.tolist())) >= dbu.GROUP_MIN_DISTINCT
    for m, c in enumerate(ctxs):
        assert par.disease_bytes(c._disease) == par.disease_bytes(par.expand_numpy(dbu.base_block(), space, thetas[m], dbu.A, dbu.V)[0])


def test_the_two_group_spaces_cover_every_field_a_knob_may_scale():
    fields = set(k.field for s in dbu.GROUP_SPACES.values() for k in s)
    assert fields == set(par.FIELDS)
