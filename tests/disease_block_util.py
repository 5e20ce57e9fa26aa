"""The case table of the disease-block parity tests: disease blocks off the bundled values, each `base * theta` on one knob or
one small family of knobs (reina_model_amd/parameters.py: expand_numpy), so that a divergence names its field.  Shared by
tests/test_disease_blocks.py (oracle B alone: every case runs a real epidemic, fails where recorded, and its block differs from
the base in the named fields only) and tests/test_disease_blocks_gpu.py (a HIP engine under block X == oracle B under block X).

Scenario: filter_util.small_scenario(20000) -- 12 beds, 2 ICU units; 39 whole tiles and 32 agents --, ipc='auto', seed 5, 60 days
compared in chunks of 20.  Base: the `_disease` of a Context of that scenario.  The recorded ends are oracle B's.

No case feeds a zero MEAN DURATION to a run: with a mean onset duration of 0 the gamma draw gives NaN onset_days on oracle B
(DESIGN.md section 6p), outside the domain of the parity guarantee."""
from datetime import date, timedelta

import numpy as np

import filter_util
import par_backend
from reina_model_amd import parameters as par
from reina_model_amd import simulation
from reina_model_amd.parameters import Knob, ParameterSpace

N_AGENTS, SEED, DAYS, CHUNK = 20000, 5, 60, 20
A, V = 101, 2
ULP = float(np.float32(1.0) + np.float32(2.0 ** -23))
FAIL_TEXT = 'Day counter overflow'
MIN_INFECTED, MIN_DEAD, MIN_VARIANT1 = 300, 10, 200
VARIANT1_IMPORT_DAY, VARIANT1_IMPORTS = 10, 400


class Case:
    """knobs + theta of one block; `recorded`: oracle B's (all_infected, dead) in the last history row of DAYS days (a failing
    case: the 0-based iterate() that raises); `deaths`: the case scales a severity or death field and must end with MIN_DEAD
    dead; `strict_days`: strict days oracle B must get through without failing (the cases close under a failing one);
    `variant1`: needs the import of variant 1 and MIN_VARIANT1 agents carrying it"""

    def __init__(self, name, knobs, theta, recorded, deaths=False, strict_days=None, variant1=False):
        self.name, self.knobs, self.theta, self.recorded = name, knobs, tuple(theta), recorded
        self.deaths, self.strict_days, self.variant1 = deaths, strict_days, variant1
        self.space = ParameterSpace(knobs)
        self.fields = tuple(sorted(set(k.field for k in knobs)))


_INC0 = lambda: [Knob('inc', 'mean_incubation_duration', variants=[0])]
_REC0 = lambda: [Knob('rec', 'mean_duration_from_onset_to_recovery', variants=[0])]

CASES = [
    Case('short incubation', _INC0(), [0.05], (1280, 13)),
    Case('tiny incubation', _INC0(), [1e-3], (1280, 13)),
    Case('long incubation', _INC0(), [8], (1290, 5), strict_days=80),
    Case('long recovery', _REC0(), [3], (9805, 190), strict_days=80),
    # both clamp to 1: severity_of's outside-hospital branch divides by 1 - 1
    Case('outside-hospital deaths clamp', [Knob('out', 'p_death_outside_hospital'), Knob('sym', 'p_symptomatic')], [1000, 1000],
         (15454, 2654), deaths=True),
    Case('severity chain clamps', [Knob('sev', 'p_severe_given_symptomatic'), Knob('crit', 'p_critical_given_severe'),
                                   Knob('fat', 'p_fatal_given_critical')], [1000, 1000, 1000], (6805, 3793), deaths=True),
    # psus_max leaves the bundled band, p above 1
    Case('susceptibility maximum moves', [Knob('kids', 'p_susceptibility', ages=(0, 19)), Knob('beta', 'infectiousness_multiplier')],
         [3, 1.7], (18215, 748)),
    Case('part of the population immune', [Knob('kids', 'p_susceptibility', ages=(0, 19))], [0], (7120, 188)),
    Case('nobody symptomatic', [Knob('sym', 'p_symptomatic')], [0], (409, 0)),
    Case('no transmission', [Knob('beta', 'infectiousness_multiplier')], [0], (390, 2)),
    Case('asymptomatic factor 0, no-bed deaths certain',
         [Knob('asym', 'p_asymptomatic_infection'), Knob('ward', 'p_hospital_death_no_beds'), Knob('icu', 'p_icu_death_no_beds')],
         [0, 1000, 1000], (9696, 439), deaths=True),
    Case('one ulp', [Knob('beta', 'infectiousness_multiplier'), Knob('sus', 'p_susceptibility')], [ULP, ULP], (9793, 238)),
    Case("variant 1's own values",
         [Knob('beta1', 'infectiousness_multiplier', variants=[1]), Knob('sus1', 'p_susceptibility', variants=[1]),
          Knob('rec1', 'mean_duration_from_onset_to_recovery', variants=[1]), Knob('death1', 'mean_duration_from_onset_to_death', variants=[1])],
         [1.4, 0.7, 1.5, 0.6], (16327, 661), deaths=True, variant1=True),
]
CASE_NAMES = [c.name for c in CASES]

# (knobs, theta, oracle B's failing iterate(), 0-based): strict runs, one iterate() at a time
FAILING = [
    Case('incubation x 30', _INC0(), [30], 4),
    Case('incubation x 12', _INC0(), [12], 18),
    Case('recovery x 4', _REC0(), [4], 28),
]
FAILING_NAMES = [c.name for c in FAILING]

# two shards on one GPU: mirror attribution is the only place the device divides p_susceptibility / psus_max
SHARDED = Case('two shards', [Knob('kids', 'p_susceptibility', ages=(0, 19)), Knob('beta', 'infectiousness_multiplier')], [3, 1.3],
               {'exact': 16548, 'mirror': 16334})
SHARDED_SEED, SHARDED_MIN_INFECTED = 4, 5000

# the group route (ensemble.run_parameter_ensemble): six members, seeds 31..36, every knob its own theta per member
GROUP_SEEDS = [31, 32, 33, 34, 35, 36]
GROUP_MIN_INFECTED, GROUP_MIN_DISTINCT = 1000, 3
# space A: the eight knobs of test_params_gpu.py, with mean_incubation_duration v1 (the incubation draw reads variant 0's mean
# only: that knob moves nothing) replaced by mean_duration_from_onset_to_recovery v0
GROUP_SPACES = {
    'A': [Knob('beta', 'infectiousness_multiplier'), Knob('asym', 'p_asymptomatic_infection', variants=[0]),
          Knob('rec', 'mean_duration_from_onset_to_recovery', variants=[0]), Knob('kids', 'p_susceptibility', variants=[0], ages=(0, 19)),
          Knob('sus1', 'p_susceptibility', variants=[1]), Knob('sym', 'p_symptomatic'),
          Knob('sev', 'p_severe_given_symptomatic', ages=(70, 100)), Knob('out', 'p_death_outside_hospital', ages=(0, 69))],
    # space B: what A leaves
    'B': [Knob('ward', 'p_hospital_death_no_beds'), Knob('icu', 'p_icu_death_no_beds'),
          Knob('inc', 'mean_incubation_duration', variants=[0]), Knob('death', 'mean_duration_from_onset_to_death', variants=[0]),
          Knob('crit', 'p_critical_given_severe'), Knob('fat', 'p_fatal_given_critical'),
          Knob('old', 'p_susceptibility', variants=[0, 1], ages=(60, 100)), Knob('beta1', 'infectiousness_multiplier', variants=[1])],
}
GROUP_RECORDED = {'A': [9857, 2924, 5231, 4433, 11332, 14470], 'B': [9857, 10879, 10911, 11284, 8622, 9654]}


def group_thetas():
    th = np.random.default_rng(5).uniform(0.4, 2.0, (6, 8)).astype(np.float32)
    th[0] = 1
    return th


def scenario():
    return filter_util.small_scenario(N_AGENTS)


_base = []


def base_block():
    """the scenario's own disease block (a block is made on the host: the engine library does not enter)"""
    if not _base:
        v, ages = scenario()
        c = simulation.make_context(v, age_counts=ages, seed=1, ipc=None, engine_factory=par_backend.par_engine_factory)
        assert (c.nr_ages, c.nr_variants) == (A, V)
        _base.append(c._disease)
    return _base[0]


def block_of(case):
    return par.expand_numpy(base_block(), case.space, case.theta, A, V)[0]


def interventions_of(case, variables):
    """None (the scenario's own), or for the variant-1 case the scenario's own and an import of variant 1 on day 10"""
    if not case.variant1:
        return None
    day = date.fromisoformat(variables['start_date']) + timedelta(days=VARIANT1_IMPORT_DAY)
    return [list(iv) for iv in variables['interventions']] + [['import-infections', day.isoformat(), VARIANT1_IMPORTS, 'b1.1.7']]


def ends(hist):
    """(all_infected, dead) of the last row of a history: the state before the last day"""
    return int(filter_util.totals(hist, 'all_infected')[-1]), int(filter_util.totals(hist, 'dead')[-1])


def carries_variant1(ctx):
    """agents that have been infected and whose hot word carries variant 1 (bits 8-9; reina_prims.h)"""
    hot = np.asarray(ctx.engine.alloc.to_host(ctx.engine.tensors['hot'])).view(np.uint32)
    return int(np.count_nonzero(((hot & 7) != 0) & (((hot >> 8) & 3) == 1)))
