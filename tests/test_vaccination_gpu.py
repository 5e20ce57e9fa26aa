"""The vaccination report on the GPU: the device route (k_vacc_report through reina_vacc_report) against the numpy specification
of the read-back state -- hot words, cold word 5, log words -- on simulated runs, on synthetic states at tile edges and of every
combination, on engine groups, on a logged particle filter, on logs begun mid-run, and the refusals through the C ABI.  The
report is a function of the state and the log, so no host-driven reference run is needed.  Exact equality of words throughout."""
import copy
import ctypes
import gc

import numpy as np
import pytest

import filter_util
import par_backend
import snap_util
import tx_util
import txlog_util as tu
import vacc_util as vu
from filter_util import small_scenario
from reina_model_amd import engine as eng
from reina_model_amd import ensemble, filtering, simulation
from reina_model_amd import vaccination as vac
from reina_model_amd.variables import VARIABLE_DEFAULTS

pytestmark = pytest.mark.gpu

DAYS = 200
FINE = np.minimum(np.arange(101) // 7, 15)   # a 16-group table


@pytest.fixture(autouse=True)
def _engines_go_with_their_test():
    """A logged Context and its log refer to each other: its engine goes only when the cycle collector runs"""
    yield
    gc.collect()


def _make(v, ages=None, seed=1, **kw):
    return simulation.make_context(v, age_counts=ages, seed=seed, ipc=None, **kw)


def _report_equals_spec(ctx, n_days=None, groups=None):
    assert ctx.transmission_log.on_device and ctx.transmission_log.device.group is None and ctx.engine.vacc_f is not None
    got = ctx.transmission_log.vaccination_report(groups, n_days)
    want = vu.spec_report(ctx, n_days, groups)
    vu.assert_words(got.words, want.words)
    assert np.array_equal(got.group_sizes, want.group_sizes)
    return got


# ---------------------------------------------------------------------------------------------- simulated runs

@pytest.mark.parametrize('env', ('REINA_DAY_MODE=dense', 'REINA_DAY_MODE=sparse', ''))
def test_mini_200_days_device_report_equals_spec(env, monkeypatch):
    if env:
        monkeypatch.setenv(*env.split('='))
    v, ages = vu.vaccination_scenario()
    ctx = _make(v, ages, 3, txlog=True)
    ctx.run(DAYS)
    r = _report_equals_spec(ctx)
    assert r.n_days == DAYS and r.undetermined == r.bad_vacc_day == r.out_of_range == 0
    assert int(r.outcome[vac.RECENT, :, 0].sum()) > 500 and int(r.outcome[vac.PROTECTED, :, 0].sum()) > 1000 and r.after_infection > 500
    if not env:
        short = _report_equals_spec(ctx, n_days=50)          # (most known days out of range)
        assert short.out_of_range > 0
        _report_equals_spec(ctx, n_days=eng.MAX_DAYS)
        fine = _report_equals_spec(ctx, groups=FINE)
        assert fine.n_groups == 15 and int(fine.vaccinations.sum()) == r.vaccinated
        _report_equals_spec(ctx, n_days=eng.MAX_DAYS, groups=FINE)
        assert r.coverage_frame().shape == (DAYS, r.n_groups)


def test_hus_200_days_with_a_mass_programme():
    v = vu.mass_programme(copy.deepcopy(VARIABLE_DEFAULTS))
    ctx = _make(v, None, 5, txlog=True)
    ctx.run(DAYS)
    r = _report_equals_spec(ctx)
    assert r.vaccinated > 1000000 and int(r.outcome[vac.PROTECTED, :, 0].sum()) > 10000 and r.undetermined == r.out_of_range == 0


# ---------------------------------------------------------------------------------------------- synthetic states

def _synthetic(hot, inf, cnt, log, vd):
    ctx = snap_util.make_context(len(hot))
    tx_util.put_forest(ctx, hot, inf, cnt)
    vu.put_vaccinations(ctx, hot, vd)
    tlog = ctx.start_transmission_log()
    assert tlog.on_device
    tlog.set_words(log)
    got_hot, got_vd = vu.host_arrays(ctx)
    assert np.array_equal(got_hot, hot) and np.array_equal(got_vd, vd)
    return ctx


def _synthetic_report(ctx, hot, log, vd, n_days, kind='default'):
    g = tx_util.groups(kind)
    got = ctx.transmission_log.vaccination_report(g, n_days)
    want = vac.report_numpy(hot, vd, log, np.asarray(ctx.engine.config.age_start), g, n_days)
    vu.assert_words(got.words, want.words)
    return got


@pytest.mark.parametrize('n', tu.SIZES)
def test_report_kernel_equals_spec_at_tile_edges(n):
    hot, inf, cnt, log, vd = vu.forest_state(n)
    ctx = _synthetic(hot, inf, cnt, log, vd)
    r = _synthetic_report(ctx, hot, log, vd, vu.N_DAYS, 'fine' if n % 2 else 'default')
    assert r.vaccinated == int(((hot & vu.VACCINATED) != 0).sum()) and r.infected == int(((hot & 7) != 0).sum())
    _synthetic_report(ctx, hot, log, vd, 1)


def test_report_kernel_equals_spec_on_every_combination():
    hot, inf, cnt, log, vd = vu.combos_state()
    ctx = _synthetic(hot, inf, cnt, log, vd)
    r = _synthetic_report(ctx, hot, log, vd, vu.N_DAYS)
    assert (r.outcome[:, :, 0].sum(axis=1) > 0).all() and all(getattr(r, name) > 0 for name in vac.SCALAR_NAMES)
    _synthetic_report(ctx, hot, log, vd, 1)
    _synthetic_report(ctx, hot, log, vd, eng.MAX_DAYS, 'fine')


@pytest.mark.parametrize('which', ('only_susceptible_vaccinated', 'nobody_vaccinated'))
def test_both_branches_of_the_tile_skip(which):
    n = tu.SIZES[-1]
    hot, inf, cnt, log, vd = vu.forest_state(n, seed=2)
    if which == 'only_susceptible_vaccinated':   # no infected agent at all; whole tiles without a vaccinated one are skipped
        hot = np.where((np.arange(n) // 512) % 2 == 0, hot & np.uint32(vu.VACCINATED), 0).astype(np.uint32)
        inf[:], cnt[:] = -1, 0
    else:
        hot = (hot & ~np.uint32(vu.VACCINATED)).astype(np.uint32)
    ctx = _synthetic(hot, inf, cnt, log, vd)
    r = _synthetic_report(ctx, hot, log, vd, vu.N_DAYS)
    if which == 'only_susceptible_vaccinated':
        assert r.infected == 0 and r.vaccinated > 100 and int(r.population[:, 1].sum()) == r.vaccinated and not r.severity.any()
    else:
        assert r.vaccinated == 0 and r.infected > 100 and int(r.outcome[vac.UNVACCINATED, :, 0].sum()) == r.infected and not r.vaccinations.any()


# ---------------------------------------------------------------------------------------------- groups

@pytest.mark.parametrize('members', (1, 3, 4))
def test_logged_groups_equal_single_contexts(members):
    v, ages = vu.vaccination_scenario(day=5)
    seeds, days = list(range(40, 40 + members)), 60
    planner = _make(v, ages, seeds[0])
    ctxs = [_make(v, ages, sd) for sd in seeds]
    ensemble.run_group_plan(ctxs, planner.make_plan(days), txlog=True)
    glog = ctxs[0].transmission_log.device
    assert glog.group is not None and all(c.transmission_log.device is glog for c in ctxs)
    reps = ensemble.vaccination_reports(ctxs)
    assert len(reps) == members
    for m, sd in enumerate(seeds):
        vu.assert_words(reps[m].words, vu.spec_report(ctxs[m]).words)
        vu.assert_words(reps[m].words, ctxs[m].transmission_log.vaccination_report().words)   # (a member's own report: the numpy route)
        solo = _make(v, ages, sd, txlog=True)
        solo.run(days)
        vu.assert_words(reps[m].words, _report_equals_spec(solo).words)
        del solo
        assert reps[m].n_days == days and int(reps[m].outcome[vac.PROTECTED, :, 0].sum()) > 0
    assert all(not np.array_equal(reps[0].words, r.words) for r in reps[1:]), 'the members differ by seed'
    fine = ensemble.vaccination_reports(ctxs, age_groups=FINE, n_days=30)
    for m in range(members):
        vu.assert_words(fine[m].words, vu.spec_report(ctxs[m], 30, FINE).words)
    for c in ctxs:
        c.transmission_log = None
    glog.close()
    glog.group.close()


def test_logged_filter_reports_every_final_particle():
    K, days, window = 4, 21, 7
    v, ages = vu.vaccination_scenario(day=2)
    truth = simulation.make_context(v, age_counts=ages, seed=777, ipc='auto', engine_factory=par_backend.par_engine_factory)
    obs = filter_util.observations(truth.run(days), v['start_date'], range(1, days))
    model = filtering.ObservationModel({'all_detected': 8.0, 'in_ward': 8.0})
    r = filtering.particle_filter(v, K, observations=obs, obs_model=model, window=window, days=days, ess_threshold=1.0,
                                  seeds=list(range(100, 100 + K)), filter_seed=5, age_counts=ages, txlog=True)
    try:
        assert len(r.windows) == 3 and r.log is not None
        reps = r.vaccination_reports()
        assert len(reps) == K
        for k, c in enumerate(r.contexts):
            vu.assert_words(reps[k].words, vu.spec_report(c, days, log_words=r.log.words(k)).words)
            assert reps[k].n_days == days and reps[k].vaccinated > 10000 and reps[k].undetermined == 0
        assert sum(int(rep.outcome[vac.RECENT, :, 0].sum()) for rep in reps) > 0
    finally:
        r.close()
    with pytest.raises(ValueError, match='closed'):
        r.vaccination_reports()


# ---------------------------------------------------------------------------------------------- logs begun mid-run

def test_log_begun_at_day_60_and_on_a_restored_context_at_day_120():
    v, ages = vu.vaccination_scenario()
    a = _make(v, ages, 3)
    a.run(60)
    a.start_transmission_log()
    a.run(DAYS - 60)
    r = _report_equals_spec(a)
    assert r.undetermined > 0 and int(r.vaccinations[:60].sum()) > 0 and int(r.infections[:60].sum()) == 0
    b = _make(v, ages, 3)
    b.run(120)
    c = _make(v, ages, 3, snapshot=b.snapshot(), txlog=True)
    assert c.day == 120 and c.transmission_log.on_device
    c.run(DAYS - 120)
    rc = _report_equals_spec(c)
    assert rc.undetermined > r.undetermined and np.array_equal(rc.vaccinations, r.vaccinations), 'the snapshot carries the cold records'
    assert np.array_equal(rc.words[vac.POPULATION:vac.SCALARS], r.words[vac.POPULATION:vac.SCALARS])


# ---------------------------------------------------------------------------------------------- refusals

def test_refusals_through_the_c_abi():
    v, ages = vu.vaccination_scenario()
    c = _make(v, ages, 1, txlog=True)
    c.run(20)
    e, dlog = c.engine, c.transmission_log.device
    f, stream, torch = e.vacc_f, e.alloc.stream(), e.alloc.torch
    UNTOUCHED = -77
    rep = torch.full((vac.report_words(4) + 2,), UNTOUCHED, dtype=torch.int64, device=e.alloc.device)
    table = np.zeros(eng.MAX_AGES, dtype=np.uint8)
    high = table.copy()
    high[5] = 3
    last = lambda: e.f['last_error']()
    for n_days in (0, eng.MAX_DAYS + 1):
        assert f['vacc_report'](dlog._h, table.ctypes.data, 1, n_days, rep.data_ptr(), stream) == -1
        assert b'vaccination report: n_days must be in [1, REINA_MAX_DAYS]' in last()
    assert f['vacc_report'](dlog._h, high.ctypes.data, 3, 4, rep.data_ptr(), stream) == -1
    assert b"vaccination report: an age's group is not below n_groups" in last()
    assert f['vacc_report'](dlog._h, table.ctypes.data, 0, 4, rep.data_ptr(), stream) == -1 and b'n_groups' in last()
    assert f['vacc_report'](dlog._h, table.ctypes.data, vac.MAX_GROUPS + 1, 4, rep.data_ptr(), stream) == -1 and b'n_groups' in last()
    assert f['vacc_report'](dlog._h, None, 1, 4, rep.data_ptr(), stream) == -1
    assert f['vacc_report'](dlog._h, table.ctypes.data, 1, 4, rep.data_ptr() + 8, stream) == -1
    assert b'vaccination report: the report must be a 16-byte aligned device buffer' in last()
    assert f['vacc_report'](dlog._h, table.ctypes.data, 1, 4, None, stream) == -1 and b'aligned' in last()
    assert f['vacc_report'](None, table.ctypes.data, 1, 4, rep.data_ptr(), stream) == -1
    torch.cuda.synchronize()
    assert bool((rep == UNTOUCHED).all()), 'a refused call queued something'
    assert f['vacc_report'](dlog._h, table.ctypes.data, 1, 4, rep.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    got = rep.cpu().numpy()
    want = vu.spec_report(c, 4, np.zeros(101, dtype=np.int64))
    vu.assert_words(got[:vac.report_words(4)].view(np.uint64), want.words)
    assert (got[vac.report_words(4):] == UNTOUCHED).all(), 'the block is report_words(n_days) words'
    # a destroyed log: the handle a closed DeviceLog is left with
    c.transmission_log.close()
    assert not dlog._h
    assert f['vacc_report'](dlog._h, table.ctypes.data, 1, 4, rep.data_ptr(), stream) == -1
    with pytest.raises(eng.EngineError):
        c.transmission_log.vaccination_report()
    # sharded engines cannot have a log
    from reina_model_amd import sharding
    members = []
    shards = [simulation.make_context(v, age_counts=ages, seed=1, ipc=None, comm=sharding.InProcessComm(k, 2, members)) for k in range(2)]
    h = ctypes.c_void_p()
    es = shards[0].engine
    assert es.txlog_f['txlog_create'](es._h, es.alloc.stream(), ctypes.byref(h)) == -1 and not h
    with pytest.raises(ValueError, match='sharded'):
        shards[0].start_transmission_log()
