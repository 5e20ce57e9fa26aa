"""GPU parity tests proper: the HIP engine (through the C ABI, libreina_hip.so) against the CPU
oracle B (oracle/reina_par.c) on the same seeded inputs.  Everything compared is integer or raw
float bits and must match EXACTLY: per-day counter blocks, the final hot words, infector links,
infection counts, onset durations, vaccination days, testing-queue contents (as sets).
"""
import copy

import numpy as np
import pytest

from golden_util import load_run, variables_for
from parity_util import _assert_bit_planes, _assert_state_equal, _pair, _run_and_compare, _sharded_pair  # noqa: F401
from reina_model_amd import datasets, simulation
from reina_model_amd import engine as eng
from reina_model_amd.variables import VARIABLE_DEFAULTS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_mini_default_scenario(seed):
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    v.update(hospital_beds=12, icu_units=2)
    _run_and_compare(v, datasets.scaled_population(20000), seed, 200)


@pytest.mark.parametrize('name', ['mini_kitchen_s0', 'mini_kitchen_s3'])
def test_mini_kitchen_sink(name):
    """all intervention types: vaccination cursors, new beds/ICU, variant imports, weekly shares,
    masks, p_icu_death_no_beds < 1"""
    _, meta = load_run(name)
    _run_and_compare(variables_for(meta), np.asarray(meta['age_counts']), meta['seed'], meta['days'],
                     interventions=meta['interventions'])


@pytest.mark.parametrize('name', ['turku_default_s0', 'turku_astra-zeneca_s1', 'turku_stop-wearing-masks_s0', 'turku_autumn_s0'])
def test_turku_override_set(name):
    """the reference's other deployment (variables.py:10-216, VARIABLE_OVERRIDE_SET=turku): 192 962 agents x 470 days -- nine
    contact-tracing steps, place-specific mask ladders, weekly imports with a variant share growing to 99 %, the `vaccinate`
    programme of the astra-zeneca scenario; `autumn`: the 2020-09-01 start with the initial condition from Turku's case rows"""
    _, meta = load_run(name)
    v = variables_for(meta)
    assert v['area_name'] == 'Turku' and v['hospital_beds'] == 900
    gpu, _ = _run_and_compare(v, np.asarray(meta['age_counts']), meta['seed'], meta['days'], interventions=meta['interventions'],
                              ipc=meta.get('ipc'), chunk=235)
    if 'astra' in name or 'autumn' in name:
        assert gpu.generate_state()['vaccinated'].sum() > 10000


def test_mini_imports_only():
    _, meta = load_run('mini_imports_s1')
    _run_and_compare(variables_for(meta), np.asarray(meta['age_counts']), meta['seed'], meta['days'],
                     interventions=meta['interventions'])


@pytest.mark.parametrize('mode', ['dense', 'sparse'])
def test_sparse_and_dense_days_are_the_same_day(mode, monkeypatch):
    """k_day streams either every hot word (dense day) or the ACTIVE bit plane and the words of the agents it names
    (sparse day, round 4) -- chosen per day from yesterday's count of active agents.  Forced one way and the other
    (REINA_DAY_MODE), every scenario family gives oracle B's results bit for bit: the mini default scenario through its
    peak (a third of the population infected -- in the sparse form every lane then queues several agents per step), all
    intervention types, population sizes that are not a multiple of 4 / of a tile, random scenarios with initial
    conditions, three variants with tracing."""
    monkeypatch.setenv('REINA_DAY_MODE', mode)
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    v.update(hospital_beds=12, icu_units=2)
    _run_and_compare(v, datasets.scaled_population(20000), 4, 200)
    _, meta = load_run('mini_kitchen_s0')
    _run_and_compare(variables_for(meta), np.asarray(meta['age_counts']), meta['seed'], meta['days'],
                     interventions=meta['interventions'])
    v.update(hospital_beds=3, icu_units=1)
    for total in (4099, 10007, 511, 513, 2049):
        _run_and_compare(v, datasets.scaled_population(total), 11, 90)
    for case in (3, 8, 14):
        rng = np.random.default_rng(1000 + case)
        vv, ages, days, ivs, ipc = _random_scenario(rng)
        _run_and_compare(vv, ages, int(rng.integers(0, 2 ** 31)), days, interventions=ivs, chunk=40, ipc=ipc)


def test_sparse_and_dense_days_mixed_in_one_run(monkeypatch):
    """The two forms of k_day's stream are two instantiations of the kernel, chosen per launch (by population size; REINA_DAY_MODE
    forces one).  REINA_DAY_MODE=alternate takes the sparse form on even days and the dense one on odd days: what one form
    leaves behind (hot words, the ACTIVE bit plane, the per-wave slices) is what the other finds.  9 M agents through the first
    wave -- oracle B's days bit for bit.  (Rounds 4-5 had one kernel deciding at run time by yesterday's count of active agents,
    REINA_DAY_SPARSE_DIV; that threshold never chose the dense form where the sparse one was possible and is gone; the count
    itself, control words REINA_L_ACTIVE, stays a caller-visible diagnostic.)"""
    import bench
    monkeypatch.setenv('REINA_DAY_MODE', 'alternate')
    vv, ages = bench.scaled_scenario(copy.deepcopy(VARIABLE_DEFAULTS), 9_000_000)
    gpu, cpu = _run_and_compare(vv, ages, 8, 150, chunk=50)
    ctl = gpu.engine.alloc.to_host(gpu.engine.tensors['control'])
    c = gpu.per_age_counters()
    # REINA_L_ACTIVE (words 24-25 by day parity): day 149's stream queued every infected agent and every removed one not yet
    # counted into R
    assert int(ctl[24 + 1]) >= int(c['infected'].sum()) - int(c['new_infections'].sum()) > 0
    assert c['all_infected'].sum() > 9_000_000 // 10


@pytest.mark.parametrize('env', ['REINA_OPEN_TICKETS', 'REINA_IMPORTS_IN_OPEN'])
def test_the_alternative_launch_shapes_of_the_opening_give_the_same_days(env, monkeypatch):
    """Two choices of round 4 have their older form behind a switch, and both forms must give oracle B's days: the roles of
    the day-opening launch by block number (a single engine, resident as a whole) or by arrival ticket (engine groups; forced
    here by REINA_OPEN_TICKETS), and the weekly imports placed beside the stream in k_day's launch or by the opening launch
    (days with intervention imports; forced by REINA_IMPORTS_IN_OPEN).  Scenarios with weekly imports, tracing at both
    levels, vaccination and an initial condition."""
    monkeypatch.setenv(env, '1')
    _, meta = load_run('mini_kitchen_s3')
    _run_and_compare(variables_for(meta), np.asarray(meta['age_counts']), meta['seed'], meta['days'], interventions=meta['interventions'])
    _, meta = load_run('mini_imports_s1')
    _run_and_compare(variables_for(meta), np.asarray(meta['age_counts']), meta['seed'], meta['days'], interventions=meta['interventions'])
    for case in (2, 5, 11):
        rng = np.random.default_rng(1000 + case)
        vv, ages, days, ivs, ipc = _random_scenario(rng)
        _run_and_compare(vv, ages, int(rng.integers(0, 2 ** 31)), days, interventions=ivs, chunk=40, ipc=ipc)
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    _run_and_compare(v, datasets.scaled_population(300000), 3, 250, chunk=125)   # (the default scenario's weekly imports from July on)
    if env == 'REINA_OPEN_TICKETS':   # (a population above 8 M agents takes the block-number roles by default, level-1 tracing in a launch of its own)
        import bench
        vv, ages = bench.scaled_scenario(copy.deepcopy(VARIABLE_DEFAULTS), 9_000_000)
        _run_and_compare(vv, ages, 5, 135, chunk=45)


@pytest.mark.parametrize('env', [{'REINA_NO_PLACE_GROUPS': '1'}, {'REINA_LDS_ROWS_CAP': '3'}, {'REINA_NO_PLACE_GROUPS': '1', 'REINA_LDS_ROWS_CAP': '3'}])
def test_the_contact_tables_fallbacks_give_the_same_days(env, monkeypatch):
    """k_day finds a contact's place from its row's place groups (five comparisons) and leaves the table entry to the contacts
    that pass the thinning -- when every row's entries are sorted by place (the reference's always are; a caller of the C ABI
    may pass any order) and every distinct row fits the LDS image.  Otherwise the full entry search serves every contact, and a
    row beyond the image is read through L2.  Both fallbacks forced here (REINA_NO_PLACE_GROUPS; REINA_LDS_ROWS_CAP = 3 of the
    default scenario's 16 contact rows and count rows), alone and together, on scenarios with mobility windows that split the
    rows, against oracle B: the same days bit for bit."""
    for k, x in env.items():
        monkeypatch.setenv(k, x)
    _, meta = load_run('mini_kitchen_s3')
    _run_and_compare(variables_for(meta), np.asarray(meta['age_counts']), meta['seed'], meta['days'], interventions=meta['interventions'])
    for case in (3, 7):
        rng = np.random.default_rng(1000 + case)
        vv, ages, days, ivs, ipc = _random_scenario(rng)
        _run_and_compare(vv, ages, int(rng.integers(0, 2 ** 31)), days, interventions=ivs, chunk=40, ipc=ipc)
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    monkeypatch.setenv('REINA_DAY_MODE', 'sparse')
    _run_and_compare(v, datasets.scaled_population(200000), 5, 160, chunk=80)
    monkeypatch.setenv('REINA_DAY_MODE', 'dense')
    _run_and_compare(v, datasets.scaled_population(200000), 6, 160, chunk=80)


def test_sparse_dense_and_mixed_years_of_the_hus_population_are_identical(monkeypatch):
    """BASELINE configs[1] (1 685 983 agents x 365 days): the year as run by default (sparse days below 2.5 % active agents,
    dense days above: both forms occur), all days dense and all days sparse give the identical history and final state;
    the default one is compared with oracle B in test_hus_full_population_full_year."""
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    ages = datasets.get_population_for_area()
    runs = {}
    for mode in ('auto', 'dense', 'sparse'):
        if mode == 'auto':
            monkeypatch.delenv('REINA_DAY_MODE', raising=False)
        else:
            monkeypatch.setenv('REINA_DAY_MODE', mode)
        ctx = simulation.make_context(v, age_counts=ages, seed=2)
        hist = ctx.run(365)
        _assert_bit_planes(ctx)
        t = ctx.engine.tensors
        runs[mode] = (hist, [ctx.engine.alloc.to_host(t[k]).copy() for k in ('hot', 'infector', 'n_infected', 'onset_days')])
        del ctx
    for mode in ('dense', 'sparse'):
        assert np.array_equal(runs['auto'][0], runs[mode][0]), mode
        for a, b in zip(runs['auto'][1], runs[mode][1]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), mode
    # (and the default year did use both forms: its active count crosses the threshold)
    A = eng.MAX_AGES
    infected = runs['auto'][0][:, 0:A].sum(axis=1)
    assert infected.min() < int(ages.sum()) // 100 and infected.max() > int(ages.sum()) // 20


def _kernels_of_a_run(ctx, days):
    ctx.engine.profile_enable(1)
    ctx.run(days)
    k = ctx.engine.profile_read_kernels()
    ctx.engine.profile_enable(False)
    return {name: n for name, (ms, n) in k.items() if n}


def test_a_small_populations_day_is_one_launch_and_the_three_launch_form_gives_the_same_days(monkeypatch):
    """Round 6: an unsharded population of at most REINA_HOSP_SMALL_AGENTS agents runs every stretch of days it is handed as ONE
    launch (k_small_days: opening, stream + contact sampling, installs + bed / ICU walk as phases between launch-wide barriers, the
    days one after the other, k_small.inc); every other test of this file that runs such a population therefore runs that kernel.  Here: (a) that it IS the kernel that runs -- and
    that vaccination days and larger populations take the three launches --, (b) the scenario families in the
    one-launch form against oracle B, (c) the HUS year in both forms: the identical history and final state.  The form is OFF by
    default: built for round 5's verdict item 2 and measured slower than the three launches a day (k_small.inc; profiles/r06_evidence/
    small_days.txt) -- these tests keep it correct behind its switch, REINA_FUSED_DAY=1."""
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    v.update(hospital_beds=12, icu_units=2)
    small = datasets.scaled_population(20000)
    # (OFF by default -- measured slower than three launches a day, k_small.inc --: the library's default is the three launches)
    k = _kernels_of_a_run(simulation.make_context(v, age_counts=small, seed=1), 30)
    assert 'k_small_day' not in k and k.get('k_day') == 30 and k.get('k_open') == 30 and k.get('k_hosp_install') == 30, k
    monkeypatch.setenv('REINA_FUSED_DAY', '1')
    k = _kernels_of_a_run(simulation.make_context(v, age_counts=small, seed=1), 30)
    # (run() hands the library 1, 2, 4, 8, 15 days: the first call's single day takes the three launches, every stretch is one launch;
    # the kind counts the DAYS of its launches)
    assert k.get('k_small_day') == 29 and k.get('k_day') == 1 and k.get('k_open') == 1 and k.get('k_hosp_install') == 1, k
    _, meta = load_run('mini_kitchen_s0')   # (vaccination programmes from day 12 on: those days take the launches, k_vaccinate between them)
    ctx = simulation.make_context(variables_for(meta), age_counts=np.asarray(meta['age_counts']), seed=meta['seed'], interventions=meta['interventions'])
    k = _kernels_of_a_run(ctx, 40)
    assert k.get('k_small_day', 0) > 0 and k.get('k_vaccinate', 0) > 0 and k['k_small_day'] + k['k_day'] == 40 and k['k_day'] >= k['k_vaccinate'], k
    import bench
    vv, big = bench.scaled_scenario(copy.deepcopy(VARIABLE_DEFAULTS), 3_000_000)
    k = _kernels_of_a_run(simulation.make_context(vv, age_counts=big, seed=1), 10)
    assert 'k_small_day' not in k and k.get('k_day') == 10, k
    # (b) the one-launch form against oracle B (every other test of this file runs the three launches)
    _run_and_compare(v, small, 2, 200)
    for name in ('mini_kitchen_s3', 'mini_imports_s1', 'mini_initial_s1', 'turku_astra-zeneca_s1'):
        _, meta = load_run(name)
        _run_and_compare(variables_for(meta), np.asarray(meta['age_counts']), meta['seed'], meta['days'], interventions=meta['interventions'],
                         ipc=meta.get('ipc'), chunk=100)
    for case in (1, 4, 9, 12):
        rng = np.random.default_rng(1000 + case)
        vv, ages, days, ivs, ipc = _random_scenario(rng)
        _run_and_compare(vv, ages, int(rng.integers(0, 2 ** 31)), days, interventions=ivs, chunk=40, ipc=ipc)
    # (c) the HUS year (BASELINE configs[1]) either way
    hus = datasets.get_population_for_area()
    runs = {}
    for fused in ('1', '0'):
        monkeypatch.setenv('REINA_FUSED_DAY', fused)
        ctx = simulation.make_context(copy.deepcopy(VARIABLE_DEFAULTS), age_counts=hus, seed=4)
        hist = ctx.run(365)
        _assert_bit_planes(ctx)
        t = ctx.engine.tensors
        runs[fused] = (hist, [ctx.engine.alloc.to_host(t[k_]).copy() for k_ in ('hot', 'infector', 'n_infected', 'onset_days')])
        del ctx
    assert np.array_equal(runs['1'][0], runs['0'][0])
    for a, b in zip(runs['1'][1], runs['0'][1]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize('wgs', ['8', '19', '64'])
def test_the_one_launch_day_on_other_numbers_of_workgroups(wgs, monkeypatch):
    """REINA_FUSED_WGS: the launch's workgroups (default 32) -- the opening's roles, the stream's slices and the installs' units
    are dealt out over whatever number there is; 19 is no multiple of anything"""
    monkeypatch.setenv('REINA_FUSED_DAY', '1')
    monkeypatch.setenv('REINA_FUSED_WGS', wgs)
    _, meta = load_run('mini_kitchen_s3')
    _run_and_compare(variables_for(meta), np.asarray(meta['age_counts']), meta['seed'], meta['days'], interventions=meta['interventions'])
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    _run_and_compare(v, datasets.scaled_population(300000), 3, 250, chunk=125)   # (the default scenario's weekly imports from July on)


def test_eager_iterate_equals_batched_run():
    """iterate()+generate_state() per day (the reference's calling pattern) == run(days)"""
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    v.update(hospital_beds=12, icu_units=2)
    ages = datasets.scaled_population(20000)
    a = simulation.make_context(v, age_counts=ages, seed=5)
    b = simulation.make_context(v, age_counts=ages, seed=5)
    hist = b.run(60)
    for d in range(60):
        assert np.array_equal(a.engine.read_counters(), hist[d])
        a.iterate()
    assert np.array_equal(a.engine.read_counters(), b.engine.read_counters())


def test_hus_full_population_full_year():
    """BASELINE config 2 as benchmarked: 1 685 983 agents, default scenario, all 365 days (first wave,
    saturated beds / ICU, contact tracing from day 118, the autumn wave, the b1.1.7 imports) --
    per-day counter blocks and the final state bit-exact vs oracle B"""
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    _run_and_compare(v, datasets.get_population_for_area(), 0, 365, chunk=73)


def test_ragged_population_sizes():
    """N not a multiple of 4 / of the wave size; single-agent ages"""
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    v.update(hospital_beds=3, icu_units=1)
    for total in (4099, 10007):
        _run_and_compare(v, datasets.scaled_population(total), 11, 120)


@pytest.mark.parametrize('total', [50_000_000, 100_000_000, 200_000_000])
def test_conservation_at_scale(total):
    """BASELINE configs[2] at full size (50 M agents), the metric's "100 M agents", and SURVEY 8d's HBM-resident point (2 x 10^8, whose
    peak days walk > 50 000 bed / ICU events in priority ranges), 365 days; no oracle run: size-independent
    properties -- every day susceptible+infected+recovered+dead == N, all_infected ==
    infected+recovered+dead, hospitalized == in_ward+in_icu, sum(daily_contacts) == exposed_per_day,
    no problem flag; and determinism: the same seed gives the identical 365-day history twice."""
    import bench
    v, ages = bench.scaled_scenario(copy.deepcopy(VARIABLE_DEFAULTS), total)
    ctx = simulation.make_context(v, age_counts=ages, seed=1)
    hist = ctx.run(365)
    peak = int(ctx.engine.alloc.to_host(ctx.engine.tensors['control'])[eng.L_HOSP_PEAK])
    # (the busiest day on which a bed or ICU unit could run out, i.e. whose events were walked in priority order)
    assert peak > (3 * 16384 if total > 100_000_000 else 2000), peak
    del ctx
    A = eng.MAX_AGES
    N = int(ages.sum())
    def tot(name):
        i = eng.C_NAMES.index(name)
        return hist[:, i * A:(i + 1) * A].sum(axis=1)
    sc = hist[:, eng.C_NR * A:]
    assert np.all(tot('susceptible') + tot('infected') + tot('recovered') + tot('dead') == N)
    assert np.all(tot('all_infected') == tot('infected') + tot('recovered') + tot('dead'))
    assert np.all(tot('hospitalized') == tot('in_ward') + tot('in_icu'))
    assert np.all(sc[:, eng.S_DAILY_CONTACTS:eng.S_DAILY_CONTACTS + 6].sum(axis=1) == sc[:, eng.S_EXPOSED_PER_DAY])
    assert tot('all_infected')[-1] > total // 10
    assert np.all(sc[:, eng.S_PROBLEM] == 0)
    again = simulation.make_context(v, age_counts=ages, seed=1).run(365)
    assert np.array_equal(hist, again)


@pytest.mark.parametrize('attribution', ['exact', 'mirror'])
def test_sharded_population_two_shards_on_one_gpu(attribution):
    """the population split over G=2 engine instances (both on this GPU, stepped in
    lock-step, phase by phase, with the collectives carried out in between) == the same on the CPU oracle.  exact: SURVEY 8
    f-4 -- global ids, contact / feedback / tracing records through the all-to-all segments; mirror: stand-in infectors"""
    from reina_model_amd import sharding
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    v.update(hospital_beds=30, icu_units=4)
    ages = datasets.scaled_population(60000)
    G = 2
    gpu, cpu = _sharded_pair(v, ages, 4, G, attribution)
    for d in range(160):
        sharding.step_shards_together(gpu)
        sharding.step_shards_together(cpu)
        if d % 20 == 19:
            for a, b in zip(gpu, cpu):
                assert np.array_equal(a.engine.read_counters(), b.engine.read_counters()), d
    for a, b in zip(gpu, cpu):
        _assert_state_equal(a, b)
    tot = sharding.reduce_counters(gpu)
    assert tot[eng.C_NAMES.index('all_infected') * eng.MAX_AGES:][:101].sum() > 5000
    if attribution == 'exact':
        from shard_util import assert_links_are_true
        info = assert_links_are_true(gpu)
        assert info['cross_shard'] > 2000


@pytest.mark.parametrize('attribution', ['exact', 'mirror'])
@pytest.mark.parametrize('case', [155, 489, 703, 822, 1008, 2034, 2058, 200812, 7, 8, 9, 10, 11])
def test_random_scenarios_on_two_to_four_shards(case, attribution):
    """The sharded leg of the randomised soak (tools/parity_soak.py ... sharded) in the suite: random scenarios on 2-4
    in-process shards, HIP == oracle B on every tenth day's counters and on the final state.  The first seven are scenarios
    on which the soak of round 3 found mismatches that did not repeat run to run -- a stale stand-in infector (mirror
    attribution, a small outbreak) that had been removed since: the R statistics of an agent first seen removed today are read
    by the launch that would add today's infection to its count.  A stand-in must not be a removed agent (k_remote.inc,
    oracle run_remote); 3200 further sharded scenarios then ran clean.  Case 200812 is the scenario on which a later soak found a
    HOLE in a source's inline infectee slots: a stand-in of TODAY that today's scan had removed (its list given up) took an
    infection count without a slot while a contact of the same morning took the next count with one -- a stand-in of any age
    must be an agent that has not been removed.
    Round 5: every case also under EXACT attribution (no stand-ins at all: the true infector's global id, the exchanges of
    include/reina_hip.h) -- bit for bit against oracle B in that mode, and the links are checked to be the true ones."""
    from reina_model_amd import sharding
    rng = np.random.default_rng(300000 + case)
    v, ages, days, ivs, ipc = _random_scenario(rng)
    G = int(rng.integers(2, 5))
    seed = int(rng.integers(0, 2 ** 31))
    if ipc is not None and v['hospital_beds'] == 0 and ipc.get('in_icu', 0) > 0:
        ipc = dict(ipc, in_icu=0)   # (refused by the reference and by both engines: tested elsewhere)
    gpu, cpu = _sharded_pair(v, ages, seed, G, attribution, ivs, ipc)
    for d in range(min(days, 100)):
        sharding.step_shards_together(gpu)
        sharding.step_shards_together(cpu)
        if d % 10 == 9:
            for a, b in zip(gpu, cpu):
                assert np.array_equal(a.engine.read_counters(), b.engine.read_counters()), d
    for a, b in zip(gpu, cpu):
        assert np.array_equal(a.engine.read_counters(), b.engine.read_counters())
        _assert_state_equal(a, b)
    if attribution == 'exact' and not sharding.reduce_counters(gpu)[eng.C_NR * eng.MAX_AGES + eng.S_PROBLEM]:
        from shard_util import assert_links_are_true
        assert_links_are_true(gpu)


def _random_scenario(rng):
    """A random but valid scenario: population size, capacities, disease tweaks and a random
    intervention schedule drawn from every intervention type."""
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    total = int(rng.integers(3000, 60000))
    v['hospital_beds'] = int(rng.integers(0, 40))
    v['icu_units'] = int(rng.integers(0, 6))
    v['p_icu_death_no_beds'] = float(rng.choice([100.0, 50.0, 0.0]))
    v['p_hospital_death_no_beds'] = float(rng.choice([20.0, 100.0, 0.0]))
    v['infectiousness_multiplier'] = float(rng.uniform(0.3, 1.2))
    v['variants'] = [{'name': 'b1.1.7', 'infectiousness_multiplier': float(rng.uniform(0.5, 1.5))}]
    days = int(rng.integers(60, 160))
    from datetime import date, timedelta
    d0 = date.fromisoformat(v['start_date'])
    def day(k):
        return (d0 + timedelta(days=int(k))).isoformat()
    ivs = [['import-infections', day(0), int(rng.integers(5, 80))]]
    places = [None, 'home', 'work', 'school', 'transport', 'leisure', 'other']
    for _ in range(int(rng.integers(4, 18))):
        t = rng.choice(['limit-mobility', 'wear-masks', 'import-infections', 'import-infections-weekly',
                        'test-all-with-symptoms', 'test-only-severe-symptoms', 'test-with-contact-tracing',
                        'vaccinate', 'build-new-hospital-beds', 'build-new-icu-units'])
        when = day(rng.integers(0, days))
        a, b = sorted(int(x) for x in rng.integers(0, 101, size=2))
        mn = None if rng.random() < 0.4 else a
        mx = None if rng.random() < 0.4 else b
        pl = places[int(rng.integers(0, len(places)))]
        if t == 'limit-mobility':
            ivs.append([t, when, int(rng.integers(0, 101)), mn, mx, pl])
        elif t == 'wear-masks':
            ivs.append([t, when, int(rng.integers(0, 101)), mn, mx, pl])
        elif t == 'import-infections':
            ivs.append([t, when, int(rng.integers(1, 60))] + (['b1.1.7'] if rng.random() < 0.3 else []))
        elif t == 'import-infections-weekly':
            ivs.append([t, when, int(rng.integers(0, 80)), int(rng.integers(0, 101))])
        elif t == 'test-only-severe-symptoms':
            ivs.append([t, when, int(rng.integers(0, 101))])
        elif t == 'test-with-contact-tracing':
            ivs.append([t, when, int(rng.integers(0, 101))])
        elif t == 'vaccinate':
            ivs.append([t, when, int(rng.integers(0, 3000)), mn, mx])
        elif t == 'build-new-hospital-beds':
            ivs.append([t, when, int(rng.integers(1, 20))])
        elif t == 'build-new-icu-units':
            ivs.append([t, when, int(rng.integers(1, 4))])
        else:
            ivs.append([t, when])
    ipc = None
    if rng.random() < 0.35:   # an initial population condition (set_initial_state)
        ipc = dict(dead=int(rng.integers(0, 6)), in_icu=int(rng.integers(0, 8)), in_ward=int(rng.integers(0, 15)),
                   confirmed_cases=int(rng.integers(0, 300)), incubating=int(rng.integers(0, 80)),
                   ill=int(rng.integers(0, 60)), recovered=int(rng.integers(0, 400)))
    return v, datasets.scaled_population(total), days, ivs, ipc


@pytest.mark.parametrize('case', range(20))
def test_random_scenarios(case):
    """Randomised scenarios (all intervention types, odd capacities incl. zero beds / ICU units,
    random age windows and places, a third of them with an initial population condition): HIP ==
    oracle B bit for bit."""
    rng = np.random.default_rng(1000 + case)
    v, ages, days, ivs, ipc = _random_scenario(rng)
    _run_and_compare(v, ages, int(rng.integers(0, 2 ** 31)), days, interventions=ivs, chunk=40, ipc=ipc)


def test_engine_group_equals_individual_members():
    """Monte-Carlo group (one launch per phase for all members, member = blockIdx.y): every
    member's per-day counters and final state == oracle B run alone with that member's seed;
    kitchen-sink scenario so every kernel (tracing, vaccination, imports, new beds) is covered."""
    import par_backend
    from reina_model_amd import ensemble
    _, meta = load_run('mini_kitchen_s0')
    v, ages, ivs = variables_for(meta), np.asarray(meta['age_counts']), meta['interventions']
    seeds = [3, 11, 12, 500, 77]
    days = meta['days']
    planner = simulation.make_context(v, age_counts=ages, seed=0, interventions=ivs)
    plan = planner.make_plan(days)
    members = [simulation.make_context(v, age_counts=ages, seed=s, interventions=ivs) for s in seeds]
    hist = ensemble.run_group_plan(members, plan)
    assert hist.shape == (len(seeds), days, eng.COUNTER_WORDS)
    for m, s in enumerate(seeds):
        cpu = simulation.make_context(v, age_counts=ages, seed=s, interventions=ivs,
                                      engine_factory=par_backend.par_engine_factory)
        hc = cpu.run(days)
        assert np.array_equal(hist[m], hc), 'member %d (seed %d)' % (m, s)
        assert np.array_equal(members[m].engine.read_counters(), cpu.engine.read_counters())
        _assert_state_equal(members[m], cpu)
    # members stay usable on their own after the group is gone (the planner keeps the scenario's
    # host-side state, so the continuation plan comes from it)
    # (member 0 took the group's contact tables from the host, the others by device-to-device broadcast)
    more = planner.make_plan(5)
    for m in (0, len(seeds) - 1):
        h1 = members[m].run_plan(more)
        cpu0 = simulation.make_context(v, age_counts=ages, seed=seeds[m], interventions=ivs,
                                       engine_factory=par_backend.par_engine_factory)
        cpu0.run(days)
        assert np.array_equal(h1, cpu0.run(5)), m


def test_history_readback_paths_agree():
    """TorchAllocator.to_host: small and huge tensors through the pageable copy, histories through pinned
    memory -- the same bytes either way."""
    import torch
    a = eng.TorchAllocator('cuda:0')
    for n in (1000, (1 << 16) - 3, (1 << 16) + 5, 3_000_000):
        t = torch.arange(n, dtype=torch.int32, device='cuda:0') * 7 - 11
        h = a.to_host(t)
        assert h.dtype == np.int32 and np.array_equal(h, t.cpu().numpy())
        h[0] = 5    # the caller owns what it gets
        assert int(t[0].item()) == -11


def test_run_ensemble_batched_equals_threaded():
    from reina_model_amd import ensemble
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    v.update(hospital_beds=12, icu_units=2)
    ages = datasets.scaled_population(30000)
    a = ensemble.run_ensemble(v, range(6), 120, age_counts=ages, batched=True, concurrent=4)
    b = ensemble.run_ensemble(v, range(6), 120, age_counts=ages, batched=False)
    assert np.array_equal(a, b)


def test_threaded_ensemble_short_histories_do_not_share_a_pinned_block():
    """A history of 34 days or fewer comes back through the small pinned block of TorchAllocator.to_host; the threaded
    ensemble reads back from several host threads at once, so that block must be per thread (round-2 advisor finding:
    with one block per process, members' short histories could be swapped or corrupted)."""
    from reina_model_amd import ensemble
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    v.update(hospital_beds=12, icu_units=2)
    ages = datasets.scaled_population(30000)
    a = ensemble.run_ensemble(v, range(16), 20, age_counts=ages, batched=True)
    for _ in range(3):
        b = ensemble.run_ensemble(v, range(16), 20, age_counts=ages, batched=False, threads=8)
        assert np.array_equal(a, b)


IPC = dict(dead=30, in_icu=12, in_ward=20, confirmed_cases=230, incubating=200, ill=150, recovered=900)


@pytest.mark.parametrize('beds,icu,n,ipc', [(9, 2, 60000, IPC), (2600, 300, 60000, IPC),
                                             (30, 5, 300000, dict(dead=300, in_icu=40, in_ward=90, confirmed_cases=4000,
                                                                  incubating=6000, ill=4000, recovered=12000))])
def test_initial_population_condition(beds, icu, n, ipc):
    """reina_set_initial_state (Population.set_initial_state, main.pyx:1452-1516): state right after
    construction and the following days, HIP == oracle B bit for bit; the third case needs two slot
    chunks and fills 20 % of a small age class."""
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    v.update(hospital_beds=beds, icu_units=icu, p_icu_death_no_beds=50.0)
    ages = datasets.scaled_population(n)
    import par_backend
    gpu = simulation.make_context(v, age_counts=ages, seed=9, ipc=ipc)
    cpu = simulation.make_context(v, age_counts=ages, seed=9, ipc=ipc, engine_factory=par_backend.par_engine_factory)
    assert np.array_equal(gpu.engine.read_counters(), cpu.engine.read_counters())
    s = gpu.generate_state()
    assert sum(s['all_detected']) == ipc['confirmed_cases'] and sum(s['in_icu']) <= ipc['in_icu']
    _assert_state_equal(gpu, cpu)
    hg, hc = gpu.run(60), cpu.run(60)
    assert np.array_equal(hg, hc)
    _assert_state_equal(gpu, cpu)


@pytest.mark.parametrize('n,ipc', [
    (2000, dict(dead=40, in_icu=30, in_ward=60, confirmed_cases=500, incubating=300, ill=400, recovered=2200)),
    (30000, dict(dead=500, in_icu=300, in_ward=900, confirmed_cases=9000, incubating=4000, ill=6000, recovered=29000))])
def test_initial_condition_with_more_slots_than_agents(n, ipc):
    """the reference draws the agents of the initial condition with replacement: with more slots than agents (3030 on
    2000; 40 700 -- three slot chunks -- on 30 000) most agents are visited several times, in slot order over many claim
    rounds, every visit moving the counters -- construction and 30 days, HIP == oracle B bit for bit"""
    import par_backend
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    v.update(hospital_beds=25, icu_units=10, p_icu_death_no_beds=50.0)
    ages = datasets.scaled_population(n)
    gpu = simulation.make_context(v, age_counts=ages, seed=21, ipc=ipc)
    cpu = simulation.make_context(v, age_counts=ages, seed=21, ipc=ipc, engine_factory=par_backend.par_engine_factory)
    cg, cc = gpu.engine.read_counters(), cpu.engine.read_counters()
    assert np.array_equal(cg, cc)
    A = eng.MAX_AGES
    slots = sum(ipc[k] for k in ('dead', 'in_icu', 'in_ward', 'incubating', 'ill', 'recovered'))
    assert cg[eng.C_NAMES.index('all_infected') * A:][:A].sum() == slots > n      # every visit counts (Population.infect)
    _assert_state_equal(gpu, cpu)
    assert np.array_equal(gpu.run(30), cpu.run(30))
    _assert_state_equal(gpu, cpu)


def test_the_hip_library_refuses_icu_patients_without_beds():
    """the same precondition at libreina_hip.so's C ABI (tests/test_oracle_par.py has oracle B's): REINA_E_INVALID with a
    message, nothing launched"""
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    v.update(hospital_beds=0, icu_units=2)
    ctx = simulation.make_context(v, age_counts=datasets.scaled_population(5000), seed=1)
    ic = eng.InitialState()
    ic.incubating, ic.recovered_without_illness, ic.ill, ic.dead, ic.in_icu, ic.in_ward = 5, 5, 3, 1, 2, 0
    ic.were_incubating, ic.confirmed_stride = 16, 1
    with pytest.raises(eng.EngineError, match='without beds'):
        ctx.engine.set_initial_state(ic)
    # a walk that stops short of the ICU slots (raw numbers with fewer recovered than incubating people: the reference walks
    # range(were_incubating()) and never reaches them, main.pyx:1456-1463) is a configuration the reference constructs
    ic.in_icu, ic.were_incubating = 2, 12
    ctx.engine.set_initial_state(ic)
    ic.in_icu, ic.were_incubating = 0, 14
    ctx.engine.set_initial_state(ic)
    ctx.run(5)


def test_large_bed_event_sets():
    """An unmitigated wave in 2.5 M agents with few beds: thousands of bed / ICU events per day
    while capacity binds, i.e. the counting-sort path of the event walk (more than 1024 ordered
    events) -- per-day counters and final state bit-exact vs oracle B."""
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    v.update(hospital_beds=900, icu_units=60)
    ivs = [['import-infections', '2020-02-19', 3000], ['import-infections', '2020-02-25', 3000, 'b1.1.7'],
           ['test-all-with-symptoms', '2020-02-20']]
    ages = datasets.scaled_population(2_500_000)
    gpu, cpu = _run_and_compare(v, ages, 3, 75, interventions=ivs, chunk=25)
    s = gpu.generate_state()
    assert s['available_hospital_beds'] == 0 and s['available_icu_units'] == 0
    c = gpu.per_age_counters()
    assert c['all_infected'].sum() > 1_000_000   # the wave is big enough for > 1024 events a day


def test_one_workgroup_event_walk_through_every_bucket_size():
    """The same unmitigated wave in 1.0 M agents: a population the ONE-workgroup event walk serves (k_hosp_install,
    16 priority buckets), whose ordered days grow from a few events per bucket (one key per lane of the wave that sorts
    the bucket) through 65-128 and 129-256 keys (two / four per lane) to more than 256 (the workgroup's network over runs
    of buckets) -- HIP == oracle B bit for bit, and the busiest ordered day really is past 256 keys a bucket."""
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    v.update(hospital_beds=360, icu_units=24, infectiousness_multiplier=1.0)
    v['p_severe'] = [[a, min(60.0, 3.0 * x)] for a, x in v['p_severe']]   # (three times the hospital traffic: 6283 events on the busiest ordered day)
    ivs = [['import-infections', '2020-02-19', 1200], ['import-infections', '2020-02-25', 1200, 'b1.1.7'],
           ['test-all-with-symptoms', '2020-02-20']]
    ages = datasets.scaled_population(1_000_000)
    gpu, cpu = _run_and_compare(v, ages, 3, 100, interventions=ivs, chunk=25)
    peak = int(gpu.engine.alloc.to_host(gpu.engine.tensors['control'])[eng.L_HOSP_PEAK])
    assert 16 * 256 < peak < 15000, peak


def test_sharded_population_at_config3_scale():
    """BASELINE configs[3] shape on one GPU: 4 shards x 25 M agents (10^8 in total) stepped in
    lock-step through the epidemic peak -- capacities of the cross-shard candidate region, the
    mirror table and the bed-event list hold (no problem flag), and agents are conserved."""
    import bench
    from reina_model_amd import sharding
    v, ages = bench.scaled_scenario(copy.deepcopy(VARIABLE_DEFAULTS), 100_000_000)
    G = 4
    members = []
    ctxs = [simulation.make_context(v, age_counts=ages, seed=2, comm=sharding.InProcessComm(r, G, members)) for r in range(G)]
    A = eng.MAX_AGES
    n = int(np.asarray(ages).sum())
    for d in range(140):
        sharding.step_shards_together(ctxs)
        if d % 35 == 34 or d == 139:
            c = sharding.reduce_counters(ctxs)
            tot = lambda name: int(c[eng.C_NAMES.index(name) * A:(eng.C_NAMES.index(name) + 1) * A].sum())
            assert tot('susceptible') + tot('infected') + tot('recovered') + tot('dead') == n, d
            for ctx in ctxs:
                ctx._raise_on_problem(ctx.engine.read_counters())
    assert tot('all_infected') > 5_000_000


@pytest.mark.parametrize('total,days', [(2_500_000, 70), (9_000_000, 45)])
def test_large_tracing_queues(total, days):
    """An unmitigated wave with contact tracing on: thousands of detections a day, so the level-0
    tracing pass spans several workgroups; below 8 M agents the level-1 list is walked by whichever
    of them finishes last (folded path of k_open), above it by a launch of its own -- both bit-exact
    vs oracle B."""
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    v.update(hospital_beds=3000, icu_units=300)
    ivs = [['import-infections', '2020-02-19', 3000], ['import-infections', '2020-02-25', 2000, 'b1.1.7'],
           ['test-all-with-symptoms', '2020-02-20'], ['test-with-contact-tracing', '2020-03-05', 70],
           ['import-infections-weekly', '2020-03-01', 700, 30]]
    ages = datasets.scaled_population(total)
    gpu, cpu = _run_and_compare(v, ages, 11, days, interventions=ivs, chunk=35)
    c = gpu.per_age_counters()
    assert c['all_detected'].sum() > 50_000   # >> 1024 queue entries on the busy days


def test_mass_vaccination_programmes_against_oracle_b():
    """HealthcareSystem.vaccinate_people (main.pyx:560-583) at a scale the other scenarios do not reach: k_vaccinate looks at
    16 x 1024 agents below a programme's cursor per step, so a day's number above 16 384 takes several steps, ends in the
    middle of one, and crosses age boundaries inside a wave -- 400 000 agents, two programmes on overlapping age ranges
    (23 000 and 9000 a day), a third that starts later and runs out of eligible agents, detections and deaths in between
    (agents skipped once stay ineligible): every day's counters incl. `vaccinated` by age, every agent's vaccination day."""
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    ivs = [['import-infections', '2020-02-19', 400], ['test-all-with-symptoms', '2020-02-22'],
           ['vaccinate', '2020-02-24', 161000, 40, 100], ['vaccinate', '2020-02-27', 63000, 60, 80],
           ['vaccinate', '2020-03-10', 350000, 12, 39], ['vaccinate', '2020-03-20', 7000, 40, 100]]
    gpu, cpu = _run_and_compare(v, datasets.scaled_population(400000), 21, 60, interventions=ivs, chunk=20)
    c = gpu.per_age_counters()
    assert c['vaccinated'].sum() > 300000


@pytest.mark.parametrize('one_wg', [False, True])
def test_one_vaccination_programme_by_a_chain_of_workgroups(one_wg, monkeypatch):
    """A day with ONE programme whose number exceeds a step of 16 384 agents is shared by a chain of workgroups, one step each,
    that pass on the number of eligible agents in front of them and, once reached, the final cursor (k_open.inc:
    pro_vaccinate_chain); the last one goes on alone when the steps did not hold enough eligible agents.  2 000 000 agents:
    60 000 a day from day 6 (five workgroups), over ages 30-100 until the range is used up and the cursor stops at its lower
    end; then 250 000 a day over ages 5-29, of whom there are fewer than a day's number at the end; an epidemic with detections
    runs beside it, so whole stretches of agents are ineligible.  Against oracle B, and with the chain switched off
    (REINA_VACC_ONE_WG) the same."""
    if one_wg:
        monkeypatch.setenv('REINA_VACC_ONE_WG', '1')
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    ivs = [['import-infections', '2020-02-19', 3000], ['test-all-with-symptoms', '2020-02-20'],
           ['vaccinate', '2020-02-24', 420000, 30, 100], ['vaccinate', '2020-03-20', 0, 30, 100], ['vaccinate', '2020-03-20', 1750000, 5, 29]]
    _run_and_compare(v, datasets.scaled_population(2000000), 4, 40, interventions=ivs, chunk=20)


@pytest.mark.parametrize('windows', ['overlapping', 'tiers'])
@pytest.mark.parametrize('one_wg', [False, True])
def test_several_vaccination_programmes_by_the_chain_of_workgroups(one_wg, windows, monkeypatch):
    """Round-4 verdict item 7 (main.pyx:560-593: the Turku / 2021 scenarios run age tiers side by side): a day with SEVERAL
    programmes, one of them above a step, runs every programme on the chain of workgroups, the launch agreeing on each
    programme's end before the next one starts -- three programmes on OVERLAPPING age windows (a person vaccinated by an
    earlier programme of the day is not eligible for a later one: the order matters), 2 500 000 agents, 60 000 + 25 000 +
    120 000 a day, one window used up on the way, a fourth small programme, an epidemic with detections beside it.  `tiers`:
    age tiers side by side (windows pairwise disjoint, so their order does not matter: every programme on workgroups of its
    own, all at once), joined later by a programme over all ages, which puts the day back on the sequential form.  Against
    oracle B's sequential loop, and with the chain switched off (REINA_VACC_ONE_WG) the same."""
    if one_wg:
        monkeypatch.setenv('REINA_VACC_ONE_WG', '1')
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    ivs = [['import-infections', '2020-02-19', 4000], ['test-all-with-symptoms', '2020-02-20'],
           ['vaccinate', '2020-02-23', 420000, 50, 100], ['vaccinate', '2020-02-23', 175000, 40, 69],
           ['vaccinate', '2020-02-26', 840000, 20, 59], ['vaccinate', '2020-03-05', 7000, 0, 100]]
    if windows == 'tiers':
        ivs = ivs[:2] + [['vaccinate', '2020-02-23', 420000, 70, 100], ['vaccinate', '2020-02-23', 175000, 50, 69],
                         ['vaccinate', '2020-02-26', 840000, 16, 49], ['vaccinate', '2020-03-12', 70000, 0, 100]]
    gpu, cpu = _run_and_compare(v, datasets.scaled_population(2500000), 8, 36, interventions=ivs, chunk=12)
    assert gpu.per_age_counters()['vaccinated'].sum() > 1_500_000


def test_a_day_stepped_twice_does_not_read_the_first_passes_vaccination_words():
    """the words the chained vaccination workgroups publish were tagged by the DAY and cleared only by k_init, so a caller
    of the C ABI that stepped the same day descriptor twice read the first pass's counts and cursor.  They carry the launch's
    sequence number now: two passes of one day vaccinate what oracle B's two passes do."""
    import par_backend
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    ivs = [['vaccinate', '2020-02-18', 350000, 20, 100]]
    ages = datasets.scaled_population(600000)
    gpu = simulation.make_context(v, age_counts=ages, seed=2, interventions=ivs)
    cpu = simulation.make_context(v, age_counts=ages, seed=2, interventions=ivs, engine_factory=par_backend.par_engine_factory)
    for ctx in (gpu, cpu):
        d, _ = ctx._build_day()
        assert d.n_vaccinations == 1 and d.vaccinations[0].nr == 50000
        ctx.engine.step_day(d)
        ctx.engine.step_day(d)   # the same day again
    assert np.array_equal(gpu.engine.read_counters(), cpu.engine.read_counters())
    va = gpu.engine.alloc.to_host(gpu.engine.tensors['vacc_day'])
    assert np.array_equal(va, np.asarray(cpu.engine.tensors['vacc_day']))
    assert int((va >= 0).sum()) == 100000


def test_a_vaccination_day_in_an_engine_group_runs_on_the_chain():
    """... and the members of an engine group chain too while the launch stays resident (12 members x 700 000 agents, 40 000 +
    20 000 a day on overlapping windows: three workgroups per member): sampled members == oracle B run alone."""
    import par_backend
    from reina_model_amd import ensemble
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    ivs = [['import-infections', '2020-02-19', 800], ['test-all-with-symptoms', '2020-02-20'],
           ['vaccinate', '2020-02-22', 280000, 45, 100], ['vaccinate', '2020-02-24', 140000, 30, 60]]
    ages = datasets.scaled_population(700000)
    seeds, days = list(range(30, 42)), 24
    planner = simulation.make_context(v, age_counts=ages, seed=0, interventions=ivs)
    plan = planner.make_plan(days)
    members = [simulation.make_context(v, age_counts=ages, seed=s, interventions=ivs) for s in seeds]
    hist = ensemble.run_group_plan(members, plan)
    cpus = {}
    for m in (0, 5, 11):
        cpu = cpus[m] = simulation.make_context(v, age_counts=ages, seed=seeds[m], interventions=ivs, engine_factory=par_backend.par_engine_factory)
        assert np.array_equal(hist[m], cpu.run(days)), 'member %d' % m
        _assert_state_equal(members[m], cpu)
    # ... and a member stepped ALONE after its group's vaccination days (round-5 advisor: the chained workgroups' published words live
    # in the member's own buffers, tagged with the launch's sequence number -- the representative's while in the group; a counter per
    # engine could come back to a value those words already hold.  The tag is drawn from one process-wide counter now.)
    plan2 = planner.make_plan(8)
    for m in (5, 11):
        h2 = members[m].run_plan(plan2)
        assert np.array_equal(h2, cpus[m].run(8)), 'member %d alone' % m
        _assert_state_equal(members[m], cpus[m])


def test_weekly_imports_of_a_caller_with_a_tight_candidate_buffer():
    """the weekly imports placed beside the stream leave their records in the shared candidate OVERFLOW
    list; a caller of the C ABI that sizes max_candidates tightly (here: no room at all above the per-wave regions) has no such
    list -- every weekly-import day then failed with CANDIDATE_OVERFLOW and dropped the imports.  The launch now places them in
    the day's opening whenever they do not fit with room to spare: same days as oracle B, no problem flag."""
    import par_backend
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    ivs = [['import-infections', '2020-02-19', 30], ['import-infections-weekly', '2020-02-22', 700, 40]]
    ages = datasets.scaled_population(300000)

    def tight(factory):
        def make(cfg, dis):
            cfg.max_candidates = cfg.max_work_items   # (the per-wave regions and nothing else)
            return factory(cfg, dis)
        return make
    gpu = simulation.make_context(v, age_counts=ages, seed=5, interventions=ivs, engine_factory=tight(lambda c, d: eng.hip_engine(c, d)))
    cpu = simulation.make_context(v, age_counts=ages, seed=5, interventions=ivs, engine_factory=tight(par_backend.par_engine_factory))
    hg, hc = gpu.run(40), cpu.run(40)
    assert np.array_equal(hg, hc)
    _assert_state_equal(gpu, cpu)
    assert gpu.per_age_counters()['all_infected'].sum() > 500


def test_three_variants():
    """wild type + two variants with their own multipliers and durations, imported by date and through
    the weekly shares (one 'variant_<name>' share per variant, common/interventions.py:300-323)"""
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    v.update(hospital_beds=15, icu_units=3)
    v['variants'] = [{'name': 'b1.1.7', 'infectiousness_multiplier': 1.3},
                     {'name': 'p.1', 'infectiousness_multiplier': 1.6, 'mean_incubation_duration': 4.0,
                      'p_asymptomatic_infection': 50.0}]
    ivs = [['import-infections', '2020-02-19', 40], ['import-infections', '2020-02-25', 30, 'b1.1.7'],
           ['import-infections', '2020-03-01', 30, 'p.1'], ['test-all-with-symptoms', '2020-02-22'],
           ['import-infections-weekly', '2020-03-05', 70, 30, 20], ['test-with-contact-tracing', '2020-03-20', 60],
           ['limit-mobility', '2020-03-25', 40], ['import-infections-weekly', '2020-04-20', 35, 0, 100]]
    gpu, cpu = _run_and_compare(v, datasets.scaled_population(50000), 17, 130, interventions=ivs, chunk=65)
    s = gpu.generate_state()
    assert set(s['infected_by_variant']) == {'wild-type', 'b1.1.7', 'p.1'}
    assert gpu.per_age_counters()['all_infected'].sum() > 3000


@pytest.mark.parametrize('import_wgs', [None, '1', '2'])
def test_more_imports_in_a_day_than_one_chunk(import_wgs, monkeypatch):
    """40 000 + 9 000 infections imported on single days into 3 M agents, plus a big weekly flow -- bit-exact vs oracle B.
    A day's imports are shared by up to 16 workgroups (the opening one and its helpers, or the weekly imports' own), each
    working in chunks of 16 384: by default one chunk over 16 workgroups; REINA_IMPORT_WGS=1: one workgroup, three chunks;
    2: two workgroups, two chunks."""
    if import_wgs is not None:
        monkeypatch.setenv('REINA_IMPORT_WGS', import_wgs)
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    v.update(hospital_beds=4000, icu_units=500)
    ivs = [['import-infections', '2020-02-19', 40000], ['import-infections', '2020-02-21', 9000, 'b1.1.7'],
           ['import-infections-weekly', '2020-02-24', 150000, 50], ['test-all-with-symptoms', '2020-02-25']]
    gpu, cpu = _run_and_compare(v, datasets.scaled_population(3_000_000), 5, 25, interventions=ivs, chunk=25)
    assert gpu.per_age_counters()['all_infected'].sum() > 300_000


@pytest.mark.parametrize('case', range(10))
def test_extreme_random_scenarios(case):
    """Small populations driven hard: imports of the order of the population (placement failures,
    susceptibles running out), infectiousness multipliers up to 3, no beds, contact tracing with full
    efficiency, everything at once -- HIP == oracle B bit for bit (or the identical failure)."""
    rng = np.random.default_rng(7000 + case)
    v, ages, days, ivs, ipc = _random_scenario(rng)
    total = int(rng.integers(600, 6000))
    ages = datasets.scaled_population(total)
    v['infectiousness_multiplier'] = float(rng.uniform(1.0, 3.0))
    v['variants'] = [{'name': 'b1.1.7', 'infectiousness_multiplier': float(rng.uniform(1.5, 3.0))}]
    v['hospital_beds'] = int(rng.integers(0, 3))
    v['icu_units'] = int(rng.integers(0, 2))
    from datetime import date, timedelta
    d0 = date.fromisoformat(v['start_date'])
    ivs = list(ivs) + [['import-infections', (d0 + timedelta(days=int(rng.integers(0, 20)))).isoformat(), int(total * rng.uniform(0.2, 1.5))],
                       ['import-infections-weekly', (d0 + timedelta(days=int(rng.integers(0, 30)))).isoformat(), int(total * rng.uniform(0.1, 2.0)), int(rng.integers(0, 101))],
                       ['test-with-contact-tracing', (d0 + timedelta(days=int(rng.integers(0, 30)))).isoformat(), 100]]
    if ipc is not None:
        ipc = {k: min(val, total // 12) for k, val in ipc.items()}
    _run_and_compare(v, ages, int(rng.integers(0, 2 ** 31)), min(days, 90), interventions=ivs, chunk=30, ipc=ipc)


def test_intervention_sweep_group():
    """config 5's intervention sweep on the GPU: three scenarios differing in their mobility / mask values
    as one engine group with per-member contact tables; each member bit-exact vs its own oracle-B run"""
    import par_backend
    from reina_model_amd import ensemble
    ages = datasets.scaled_population(40000)

    def scenario(scale, masks):
        v = copy.deepcopy(VARIABLE_DEFAULTS)
        v.update(hospital_beds=20, icu_units=3)
        ivs = []
        for iv in v['interventions']:
            iv = list(iv)
            if iv[0] == 'limit-mobility':
                iv[2] = int(iv[2] * scale)
            if iv[0] == 'wear-masks':
                iv[2] = masks
            ivs.append(iv)
        v['interventions'] = ivs
        return v

    vs = [scenario(1.0, 80), scenario(0.5, 30), scenario(0.25, 100)]
    seeds = [5, 5, 9]
    hist, ctxs = ensemble.run_sweep(vs, seeds, 200, age_counts=ages)
    for m in range(3):
        cpu = simulation.make_context(vs[m], age_counts=ages, seed=seeds[m], engine_factory=par_backend.par_engine_factory)
        assert np.array_equal(hist[m], cpu.run(200)), m
        _assert_state_equal(ctxs[m], cpu)


def test_more_bed_events_in_a_day_than_one_pass_holds():
    """20 M agents, unmitigated wave, scarce beds: at the peak far more than 16 384 bed / ICU events a day,
    walked in priority ranges with the free-bed / free-unit counts carried from range to range -- per-day
    counters and final state bit-exact vs oracle B's single sorted walk"""
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    v.update(hospital_beds=20000, icu_units=1500)
    ivs = [['import-infections', '2020-02-19', 40000], ['import-infections', '2020-02-22', 30000, 'b1.1.7'],
           ['test-all-with-symptoms', '2020-02-20']]
    ages = datasets.scaled_population(20_000_000)
    gpu, cpu = _run_and_compare(v, ages, 8, 70, interventions=ivs, chunk=35)
    c = gpu.per_age_counters()
    assert c['all_infected'].sum() > 10_000_000 and c['dead'].sum() > 50_000
    peak = int(gpu.engine.alloc.to_host(gpu.engine.tensors['control'])[eng.L_HOSP_PEAK])
    assert peak > 2 * 16384, peak


def test_large_engine_group_geometry():
    """64 members: each gets n_cus / 64 = 4 k_day workgroups and its share of the k_hosp_install workgroups
    (reina_hip.hip: day_blocks_for), tables arrive by broadcast -- sampled members == oracle B run alone, bit
    for bit."""
    import par_backend
    from reina_model_amd import ensemble
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    v.update(hospital_beds=40, icu_units=5)
    ages = datasets.scaled_population(70000)
    ivs = [['import-infections', '2020-02-19', 300], ['test-all-with-symptoms', '2020-02-20'], ['test-with-contact-tracing', '2020-03-05', 40],
           ['limit-mobility', '2020-03-01', 30], ['limit-mobility', '2020-03-12', 50, 0, 70, 'leisure']]
    days, K = 60, 64
    planner = simulation.make_context(v, age_counts=ages, seed=0, interventions=ivs)
    plan = planner.make_plan(days)
    members = [simulation.make_context(v, age_counts=ages, seed=900 + s, interventions=ivs) for s in range(K)]
    hist = ensemble.run_group_plan(members, plan)
    for m in (0, 1, 31, 63):
        cpu = simulation.make_context(v, age_counts=ages, seed=900 + m, interventions=ivs,
                                      engine_factory=par_backend.par_engine_factory)
        assert np.array_equal(hist[m], cpu.run(days)), m
        _assert_state_equal(members[m], cpu)
    A = eng.MAX_AGES
    i = eng.C_NAMES.index('all_infected')
    assert hist[:, -1, i * A:(i + 1) * A].sum(axis=1).min() > 300


def test_config3_at_full_size_eight_shards_of_fifty_million():
    """BASELINE configs[3] at its stated size on ONE GPU: 4 x 10^8 agents as 8 in-process shards of 5 x 10^7
    (about 40 GB of HBM), stepped in lock-step with the pressure buffers summed in between.  The first 40
    days bit for bit against oracle B sharded the same way (per-shard counter blocks; the imports are
    scaled with the population, so thousands are infected by then), then on through all 365 days:
    conservation over the shards, no problem flag, capacities of the cross-shard candidate region, the
    mirror table and the bed-event lists hold."""
    import bench
    import par_backend
    from reina_model_amd import sharding
    v, ages = bench.scaled_scenario(copy.deepcopy(VARIABLE_DEFAULTS), 400_000_000)
    G = 8
    gm, cm = [], []
    gpu = [simulation.make_context(v, age_counts=ages, seed=6, comm=sharding.InProcessComm(r, G, gm)) for r in range(G)]
    assert min(c.total_people for c in gpu) >= 49_999_900
    cpu = [simulation.make_context(v, age_counts=ages, seed=6, comm=sharding.InProcessComm(r, G, cm),
                                   engine_factory=par_backend.par_engine_factory) for r in range(G)]
    for d in range(40):
        sharding.step_shards_together(gpu)
        sharding.step_shards_together(cpu)
        if d % 10 == 9:
            for a, b in zip(gpu, cpu):
                assert np.array_equal(a.engine.read_counters(), b.engine.read_counters()), d
    for a, b in zip(gpu, cpu):
        for name in ('hot', 'infector', 'n_infected'):
            assert np.array_equal(a.engine.alloc.to_host(a.engine.tensors[name]).view(np.uint32),
                                  np.asarray(b.engine.tensors[name]).view(np.uint32)), name
    del cpu, cm
    A = eng.MAX_AGES
    n = int(np.asarray(ages).sum())
    tot = None
    # ... and on through the WHOLE year (round 4: sparse days make it cheap): the first wave, tracing from day 118, the weekly
    # imports, the autumn wave -- conservation over the shards, hospital identities, no problem flag on any shard
    for d in range(40, 365):
        sharding.step_shards_together(gpu)
        if d % 30 == 9 or d == 129 or d == 364:
            c = sharding.reduce_counters(gpu)
            tot = lambda name: int(c[eng.C_NAMES.index(name) * A:(eng.C_NAMES.index(name) + 1) * A].astype(np.int64).sum())
            assert tot('susceptible') + tot('infected') + tot('recovered') + tot('dead') == n, d
            assert tot('all_infected') == tot('infected') + tot('recovered') + tot('dead'), d
            assert tot('hospitalized') == tot('in_ward') + tot('in_icu'), d
            for ctx in gpu:
                ctx._raise_on_problem(ctx.engine.read_counters())
            if d == 129:
                assert tot('all_infected') > 20_000_000
    assert tot('all_infected') > 60_000_000 and tot('all_detected') > 20_000_000


def test_config2_fifty_million_agents_against_oracle_b():
    """BASELINE configs[2] at its stated size (5 x 10^7 synthetic agents, one GPU): the first 250 days of the scaled default
    scenario -- through the peak of the first wave, with beds and ICU units saturated and the ordered event walk of a large
    population on every one of those days; contact tracing from day 118; from day 134 the WEEKLY IMPORTS placed beside the
    stream by several import workgroups (k_open.inc: day_imports_block -- round 4's code, until now compared with the oracle
    only at HUS size, at 9 M agents and sharded: round-4 verdict item 5a); the start of the autumn wave -- per-day counter
    blocks and the final per-agent state bit for bit against oracle B (about a minute of CPU)."""
    import bench
    v, ages = bench.scaled_scenario(copy.deepcopy(VARIABLE_DEFAULTS), 50_000_000)
    gpu, cpu = _run_and_compare(v, ages, 0, 250, chunk=125)
    c = gpu.per_age_counters()
    assert c['all_infected'].sum() > 5_000_000
    peak = int(gpu.engine.alloc.to_host(gpu.engine.tensors['control'])[eng.L_HOSP_PEAK])
    assert peak > 10_000, peak   # the ordered walk really ran on a day with tens of thousands of events


def test_two_hundred_million_agents_against_oracle_b():
    """SURVEY 8d's HBM-resident point, 2 x 10^8 agents unsharded -- the one size of the bench line that had no oracle
    comparison at all (round-4 verdict item 5b): the first 130 days of the scaled default scenario (round 5: 40 days; round 6:
    through the peak -- 1.6 x 10^7 agents infected at once, the pooled beds and ICU units saturated, contact tracing), every day's
    counter block and the final per-agent state bit for bit against oracle B."""
    import bench
    v, ages = bench.scaled_scenario(copy.deepcopy(VARIABLE_DEFAULTS), 200_000_000)
    gpu, cpu = _run_and_compare(v, ages, 0, 130, chunk=65)   # (round 6: through the peak, like the other sizes of the bench line)
    c = gpu.per_age_counters()
    assert c['all_infected'].sum() > 20_000_000


def test_sharded_hundred_million_through_the_saturated_peak_against_oracle_b():
    """BASELINE configs[3] shape on one GPU: 4 shards x 25 M agents stepped in lock-step for 110 days -- the cross-shard
    pressure, the mirror tables, the demand-proportional split of the pooled beds / ICU units while they are SATURATED
    (days 85-110) and every shard's ordered event walk -- per-shard counter blocks every tenth day and the final per-agent
    state bit for bit against oracle B sharded the same way.  (Round 2's suite compared the sharded engine with the oracle
    for the first 40 days only, before the wave.)"""
    import bench
    import par_backend
    from reina_model_amd import sharding
    G, days = 4, 110
    v, ages = bench.scaled_scenario(copy.deepcopy(VARIABLE_DEFAULTS), 100_000_000)
    gpu, cpu = _sharded_pair(v, ages, 6, G, 'mirror')
    for d in range(days):
        sharding.step_shards_together(gpu)
        sharding.step_shards_together(cpu)
        if d % 10 == 9 or d == days - 1:
            for a, b in zip(gpu, cpu):
                assert np.array_equal(a.engine.read_counters(), b.engine.read_counters()), 'day %d' % d
    for a, b in zip(gpu, cpu):
        _assert_state_equal(a, b)
        # every shard has been through days on which its share of the beds / ICU units could run out (ordered walks of
        # thousands of events): the saturated regime was reached
        peak = int(a.engine.alloc.to_host(a.engine.tensors['control'])[eng.L_HOSP_PEAK])
        assert peak > 2000, peak



def test_the_metrics_hundred_million_agents_against_oracle_b():
    """The size BASELINE.json's metric is quoted on -- 10^8 synthetic agents on ONE GPU, unsharded: ALL 365 days of the
    scaled default scenario (rounds 3-5: the first 130; the peak, the summer's weekly imports beside the stream, the autumn wave --
    the peak: 8 x 10^6 agents infected at once, pooled beds and ICU units saturated, the
    ordered event walk over a thousand priority buckets, three weeks of contact tracing), every day's counter block and the
    final per-agent state bit for bit against oracle B (round-3 verdict, item 3a; about 80 s of CPU).  Every day of it is a
    sparse day (round 4): the stream reads the ACTIVE bit plane, not the hot words."""
    import bench
    v, ages = bench.scaled_scenario(copy.deepcopy(VARIABLE_DEFAULTS), 100_000_000)
    gpu, cpu = _run_and_compare(v, ages, 0, 365, chunk=73)   # (round 6: the whole year the bench line's full_scenario times)
    c = gpu.per_age_counters()
    assert c['all_infected'].sum() > 20_000_000
    peak = int(gpu.engine.alloc.to_host(gpu.engine.tensors['control'])[eng.L_HOSP_PEAK])
    assert peak > 20_000, peak


@pytest.mark.parametrize('attribution', ['exact', 'mirror'])
def test_north_stars_target_configuration_a_whole_year_on_eight_shards_against_oracle_b(attribution):
    """BASELINE.json's target configuration -- 10^8 agents over 8 GPUs -- as 8 in-process shards of 12.5 M agents on one GPU,
    ALL 365 days of the scaled default scenario: the first wave with the ONE pool of beds and ICU units saturated across
    the shards, contact tracing at 30 % from day 118, the weekly imports from July on, the autumn
    wave and the b1.1.7 imports -- every shard's counter block every tenth day and the final per-agent state of every
    shard bit for bit against oracle B sharded the same way (round-3 verdict, item 3b: no sharded run at scale had been
    stepped, let alone compared, beyond day 130).  Round 5 (verdict item 1): under EXACT attribution -- contact records,
    feedback and, from day 118, two levels of tracing requests through the all-to-all segments, every link the true one --
    and under mirror attribution as before.  (Oracle B's shards run their phases on a thread each.)"""
    import bench
    from concurrent.futures import ThreadPoolExecutor
    from reina_model_amd import sharding
    G, days = 8, 365
    v, ages = bench.scaled_scenario(copy.deepcopy(VARIABLE_DEFAULTS), 100_000_000)
    gpu, cpu = _sharded_pair(v, ages, 9, G, attribution)
    with ThreadPoolExecutor(G) as pool:
        for d in range(days):
            sharding.step_shards_together(gpu)
            sharding.step_shards_together(cpu, pool)
            if d % 10 == 9 or d == days - 1:
                for a, b in zip(gpu, cpu):
                    assert np.array_equal(a.engine.read_counters(), b.engine.read_counters()), 'day %d' % d
    tot = sharding.reduce_counters(gpu)
    A = eng.MAX_AGES
    i_all = eng.C_NAMES.index('all_infected')
    assert tot[i_all * A:(i_all + 1) * A].sum() > 15_000_000
    i_det = eng.C_NAMES.index('all_detected')
    assert tot[i_det * A:(i_det + 1) * A].sum() > 5_000_000
    for a, b in zip(gpu, cpu):
        _assert_state_equal(a, b)
        assert int(a.engine.read_counters()[eng.C_NR * A + eng.S_PROBLEM]) == 0
    if attribution == 'exact':
        from shard_util import assert_links_are_true
        info = assert_links_are_true(gpu)
        assert info['cross_shard'] > 10_000_000 and info['listed'] > 1_000_000


def test_config5_per_gpu_batch_of_128_hus_members():
    """BASELINE config 5's per-GPU batch: 128 seeds x HUS 1 685 983 agents as ONE engine group (one launch
    per phase for all 128; the day-opening launch is 128 x 66 workgroups whose roles are handed out by
    arrival tickets), 150 days = through the first wave's peak with saturated ICU -- sampled members ==
    oracle B run alone with that seed, bit for bit, final state included."""
    import par_backend
    from reina_model_amd import ensemble
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    ages = datasets.get_population_for_area()
    days, K = 150, 128
    planner = simulation.make_context(v, age_counts=ages, seed=0)
    plan = planner.make_plan(days)
    members = [simulation.make_context(v, age_counts=ages, seed=4000 + s) for s in range(K)]
    hist = ensemble.run_group_plan(members, plan)
    assert hist.shape == (K, days, eng.COUNTER_WORDS)
    for m in (0, 77, 127):
        cpu = simulation.make_context(v, age_counts=ages, seed=4000 + m, engine_factory=par_backend.par_engine_factory)
        assert np.array_equal(hist[m], cpu.run(days)), m
        _assert_state_equal(members[m], cpu)
    A = eng.MAX_AGES
    i = eng.C_NAMES.index('all_infected')
    assert hist[:, -1, i * A:(i + 1) * A].sum(axis=1).min() > 100_000


def test_the_history_comes_back_the_same_by_kernel_and_by_copies(monkeypatch):
    """reina_read_history (round 5): a page-locked destination is written by one small kernel over the link, anything else -- and every
    destination under REINA_EXPORT=memcpy -- by two copies.  Same rows, same final counter block, through all three: the kernel
    (engine.py's page-locked block), the copies forced, and a pageable numpy array handed to the library directly."""
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    v.update(hospital_beds=12, icu_units=2)
    ages = datasets.scaled_population(30000)
    days = 37   # (an odd number of rows: the copy goes 16 bytes at a time)

    def one(force_copies):
        if force_copies:
            monkeypatch.setenv('REINA_EXPORT', 'memcpy')
        else:
            monkeypatch.delenv('REINA_EXPORT', raising=False)
        ctx = simulation.make_context(v, age_counts=ages, seed=5)
        hist = ctx.run(days, record_history=True)
        return ctx, np.array(hist)

    ctx_k, by_kernel = one(False)
    ctx_c, by_copies = one(True)
    assert by_kernel.shape == (days, eng.COUNTER_WORDS) and np.array_equal(by_kernel, by_copies)
    assert by_kernel.any() and not np.array_equal(by_kernel[0], by_kernel[-1])   # (rows of a running epidemic, not a block of zeros)
    # a pageable destination: the library's own fallback, on the engine that writes by kernel otherwise
    e = ctx_k.engine
    dev = e.alloc.empty(4 * eng.COUNTER_WORDS, np.int32)
    out = np.zeros(2 * eng.COUNTER_WORDS, dtype=np.int32)
    e._check(e.f['read_history'](e._h, e.alloc.ptr(dev), 0, out.ctypes.data, e.alloc.stream()), 'read_history')
    assert np.array_equal(out[:eng.COUNTER_WORDS], e.read_counters())


def test_driver_contract_on_the_hip_engine():
    """SURVEY 8 f-3 through libreina_hip.so: simulate_individuals' (df, adf) (calc/simulation.py:148-290), the
    step_callback protocol incl. interruption, sample_model_parameters (:293-347) and run_monte_carlo
    (:349-385) give the SAME frames on the HIP engine as on the oracle-B engine."""
    import pandas as pd
    import par_backend
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    v.update(hospital_beds=12, icu_units=2, simulation_days=90, random_seed=77)
    ages = datasets.scaled_population(20000)
    df_g, adf_g = simulation.simulate_individuals(v, age_counts=ages)
    df_c, adf_c = simulation.simulate_individuals(v, age_counts=ages, engine_factory=par_backend.par_engine_factory)
    cols = [c for c in df_g.columns if c != 'us_per_infected']   # (wall-clock column)
    pd.testing.assert_frame_equal(df_g[cols], df_c[cols])
    pd.testing.assert_frame_equal(adf_g, adf_c)
    assert df_g['all_infected'].iloc[-1] > 500 and adf_g.shape == (90, 12 * 9)
    # ... and the frames have the layout of the frames the REFERENCE's own driver returned with the real cythonsim behind it
    # (tests/golden/frames_ref.json, recorded by tests/golden/_harness/make_frames_fixture.py; the values of that recording
    # are compared in tests/test_host_logic.py)
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'frames_ref.json')) as fh:
        ref = json.load(fh)
    for df_x, adf_x in ((df_g, adf_g),):
        assert list(df_x.columns) == ref['df']['columns'] and [str(t) for t in df_x.dtypes] == ref['df']['dtypes']
        assert type(df_x.index).__name__ == ref['df']['index_type'] and df_x.index.name == ref['df']['index_name']
        assert str(df_x.index.freqstr) == ref['df']['index_freq'] and str(df_x.index.dtype) == ref['df']['index_dtype']
        assert [list(c) for c in adf_x.columns] == ref['adf']['columns'] and list(adf_x.columns.names) == ref['adf']['column_names']
        assert sorted(set(str(t) for t in adf_x.dtypes)) == ref['adf']['dtypes'] and adf_x.index.name == ref['adf']['index_name']
    # the callback path: frames grow by `callback_day_interval` rows, same numbers; returning False interrupts
    seen = []

    def cb(df):
        seen.append(int(df['infected'].notna().sum()))
        return True

    df_s, adf_s = simulation.simulate_individuals(v, age_counts=ages, step_callback=cb, callback_day_interval=7)
    assert seen == list(range(7, 90, 7)) + [90]
    pd.testing.assert_frame_equal(df_s[cols], df_c[cols])
    pd.testing.assert_frame_equal(adf_s, adf_c)
    calls = []
    with pytest.raises(simulation.ExecutionInterrupted):
        simulation.simulate_individuals(v, age_counts=ages, step_callback=lambda df: calls.append(1) or len(calls) < 3,
                                        callback_day_interval=10)
    assert len(calls) == 3
    # sample_model_parameters: host-side samplers of the same library, identical Series
    for what, age, sev in (('contacts_per_day', 35, None), ('symptom_severity', 70, None), ('incubation_period', 50, None),
                           ('illness_period', 50, 'MILD'), ('hospitalization_period', 60, 'SEVERE'), ('icu_period', 60, 'CRITICAL'),
                           ('onset_to_removed_period', 80, 'FATAL'), ('infectiousness', 30, None)):
        a = simulation.sample_model_parameters(what, age, sev, variables=v)
        b = simulation.sample_model_parameters(what, age, sev, variables=v, engine_factory=par_backend.par_engine_factory)
        pd.testing.assert_series_equal(a, b)
    # run_monte_carlo: 5 seeds in groups of 4 (one full group, one of a single member)
    mc_g = simulation.run_monte_carlo('default', seeds=range(300, 305), group_size=4, days=60, write_csv=False,
                                      age_counts=ages, variables=v)
    mc_c = simulation.run_monte_carlo('default', seeds=range(300, 305), group_size=4, days=60, write_csv=False,
                                      age_counts=ages, variables=v, engine_factory=par_backend.par_engine_factory)
    mcols = [c for c in mc_g.columns if c != 'us_per_infected']
    pd.testing.assert_frame_equal(mc_g[mcols], mc_c[mcols])
    assert sorted(mc_g['run'].unique()) == list(range(300, 305)) and len(mc_g) == 5 * 60


def test_strict_iterate_raises_on_the_day_of_the_problem():
    """main.pyx:2017-2018: the reference raises SimulationFailed at the end of the iterate() that hit the
    problem.  With strict=True this engine does too (default: at the next generate_state()).  Quirk Q8
    supplies a reproducible failure: a queued agent that is hospitalised the same day is detected twice ->
    'Wrong state'; oracle B fails on the same day."""
    import par_backend
    from reina_model_amd.model import SimulationFailed
    rng = np.random.default_rng(4242)
    found = None
    for case in range(40):   # the extreme random scenarios hit the reference's own failure modes regularly
        r2 = np.random.default_rng(7000 + case)
        v, ages, days, ivs, ipc = _random_scenario(r2)
        total = int(r2.integers(600, 6000))
        ages = datasets.scaled_population(total)
        v['infectiousness_multiplier'] = float(r2.uniform(1.0, 3.0))
        v['hospital_beds'] = 0
        v['icu_units'] = 0
        from datetime import date, timedelta
        d0 = date.fromisoformat(v['start_date'])
        ivs = list(ivs) + [['import-infections', d0.isoformat(), int(total * 0.5)],
                           ['test-with-contact-tracing', (d0 + timedelta(days=2)).isoformat(), 100]]
        cpu = simulation.make_context(v, age_counts=ages, seed=case, interventions=ivs, engine_factory=par_backend.par_engine_factory, strict=True)
        fail_day = None
        for d in range(80):
            try:
                cpu.iterate()
            except SimulationFailed as e:
                fail_day = (d, str(e))
                break
        if fail_day is not None:
            found = (v, ages, ivs, case, fail_day)
            break
    assert found is not None, 'no failing scenario among the candidates'
    v, ages, ivs, case, (day, msg) = found
    gpu = simulation.make_context(v, age_counts=ages, seed=case, interventions=ivs, strict=True)
    for d in range(day):
        gpu.iterate()
    with pytest.raises(SimulationFailed) as ei:
        gpu.iterate()
    assert str(ei.value) == msg
    # default mode: the same day's iterate() returns, the problem surfaces at the next state export
    lazy = simulation.make_context(v, age_counts=ages, seed=case, interventions=ivs)
    for d in range(day + 1):
        lazy.iterate()
    with pytest.raises(SimulationFailed):
        lazy.generate_state()


@pytest.mark.parametrize('attachment', ['plain', 'txlog', 'policy'])
def test_every_route_of_the_day_runner_gives_the_same_days(attachment):
    """70 days of the default scenario (chunks of 1 + 2 + 4 + 8 + 16 + 32 + 7 days, cut once more wherever the tables change)
    by Context.run, by make_plan + run_plan, and as both members -- two Contexts of one seed -- of an engine group: identical
    histories and identical final hot words, infector links, infection counts and onset durations, word for word; plain, with
    a transmission log, and under a policy that never triggers."""
    from policy_util import never_policy
    from reina_model_amd import ensemble
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    v.update(hospital_beds=12, icu_units=2)
    ages, days, seed = datasets.scaled_population(20000), 70, 3
    policy = never_policy() if attachment == 'policy' else None
    log = attachment == 'txlog'
    make = lambda **kw: simulation.make_context(v, age_counts=ages, seed=seed, **kw)
    plan = make().make_plan(days, policy=policy)
    runs = {}
    ctx = make(policy=policy, txlog=log)
    runs['run'] = (ctx, ctx.run(days))
    ctx = make(policy=policy, txlog=log)
    runs['run_plan'] = (ctx, ctx.run_plan(plan))
    members = [make(), make()]
    hist = ensemble.run_group_plan(members, plan, policy=policy, txlog=log)
    runs['member 0'], runs['member 1'] = (members[0], hist[0]), (members[1], hist[1])
    state = lambda c: [c.engine.alloc.to_host(c.engine.tensors[k]).view(np.uint32).copy()
                       for k in ('hot', 'infector', 'n_infected', 'onset_days')]
    want_hist, want_state = np.asarray(runs['run'][1]), state(runs['run'][0])
    assert want_hist.shape == (days, eng.COUNTER_WORDS) and want_hist[-1, eng.C_NAMES.index('all_infected') * eng.MAX_AGES:][:eng.MAX_AGES].sum() > 0
    for name, (c, h) in runs.items():
        assert np.array_equal(np.asarray(h), want_hist), 'history of %s' % name
        for k, a, b in zip(('hot', 'infector', 'n_infected', 'onset_days'), state(c), want_state):
            assert np.array_equal(a, b), '%s of %s' % (k, name)
        assert c.day == days and len(c.mobility_history) == days
        if policy is not None:
            assert not np.asarray(c.policy_levels).any()
