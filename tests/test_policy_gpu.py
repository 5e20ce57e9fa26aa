"""Triggered interventions on the GPU: the device route (k_policy ahead of every day, one wait at the end) against the plain
formulation (policy.run_host_driven: one round trip a day) on a second GPU Context and on oracle B.  Exact equality
throughout.  The scenarios, policies and thresholds are those of tests/policy_util.py; tests/test_policy.py asserts on
oracle B that they switch the way these tests need."""
import ctypes

import numpy as np
import pytest

import policy_util as pu
from par_backend import par_engine_factory
from reina_model_amd import engine as eng
from reina_model_amd import ensemble, policy as pol

pytestmark = pytest.mark.gpu


def _same_history(ha, hb, what='history'):
    bad = np.argwhere(np.asarray(ha) != np.asarray(hb))
    assert len(bad) == 0, '%s: %d words differ, first at %s' % (what, len(bad), bad[0])


# ---------------------------------------------------------------------------------------------- 6. one engine, a year

def test_hus_year_device_equals_host_driven_equals_oracle():
    v, p = pu.hus_variables(), pu.ward_policy()
    dev = pu.make(v, policy=p)
    assert dev.engine.policy_f is not None
    hd = dev.run(pu.HUS_DAYS)
    host = pu.make(v)
    hh = pol.run_host_driven(host, p, pu.HUS_DAYS)
    pu.assert_same_run(dev, host, hd, hh, planes=True)
    ora = pu.make(v, factory=par_engine_factory)
    ho = pol.run_host_driven(ora, p, pu.HUS_DAYS)
    pu.assert_same_run(dev, ora, hd, ho, planes=False)
    up, down = pu.switches(dev.policy_levels)
    assert len(up) >= 2 and len(down) >= 1
    # the signal the kernel traced is the one the rule is defined on
    ward = np.asarray(hd)[:, eng.C_NAMES.index('in_ward') * eng.MAX_AGES:][:, :eng.MAX_AGES].sum(axis=1)
    assert np.array_equal(dev.policy_signal, ward)


# ---------------------------------------------------------------------------------------------- 7. groups

def _group_against_singles(v, ages, p, days):
    hist, levels, ctxs = ensemble.run_policy_ensemble(v, pu.GROUP_SEEDS, days, p, age_counts=ages)
    assert hist.shape[:2] == (32, days) and levels.shape == (32, days)
    for m, sd in enumerate(pu.GROUP_SEEDS):
        solo = pu.make(v, ages, seed=sd, policy=p)
        hs = solo.run(days)
        _same_history(hist[m], hs, 'member %d' % m)
        assert np.array_equal(levels[m], solo.policy_levels), 'member %d levels' % m
        assert list(ctxs[m].mobility_history) == list(solo.mobility_history)
        if m % 8 == 0:
            from filter_util import assert_same_day_state
            assert_same_day_state(ctxs[m], solo)
        del solo
    return levels


def test_mini_group_members_switch_on_their_own_days():
    v, ages = pu.mini_scenario()
    levels = _group_against_singles(v, ages, pu.mini_policy(), pu.MINI_DAYS)
    firsts = [pu.first_escalation(lv) for lv in levels]
    assert len(set(f for f in firsts if f >= 0)) >= 3 and firsts.count(-1) >= 1, firsts


def test_hus_group_equals_single_engines():
    levels = _group_against_singles(pu.hus_variables(), None, pu.ward_policy(), pu.GROUP_HUS_DAYS)
    assert levels.max() == 2


# ---------------------------------------------------------------------------------------------- 8. row structure (the LDS carve)

def test_levels_of_differing_row_structure():
    v, p = pu.hus_variables(), pu.rows_policy()
    dev = pu.make(v, policy=p)
    hd = dev.run(pu.HUS_DAYS)
    host = pu.make(v)
    hh = pol.run_host_driven(host, p, pu.HUS_DAYS)
    pu.assert_same_run(dev, host, hd, hh, planes=True)
    assert set(dev.policy_levels) == {0, 1, 2}


# ---------------------------------------------------------------------------------------------- 9. dated changes, masks

@pytest.mark.parametrize('start, every', [('2020-05-30', 7), ('2020-05-27', 7), ('2020-05-30', 1)])
def test_dated_table_change_on_and_off_a_review_day(start, every):
    """2020-05-30 (day 102) rebuilds the dated tables: the level is decided that very day (a review day) / three days earlier
    and is in force when the new bank arrives (no review that day) / reviewed daily"""
    v, ages = pu.mini_scenario()
    p = pol.Policy(pol.Signal('infected'), [[], [['limit-mobility', 30], ['wear-masks', 50]]], up=[0], down=[0], start=start, review_every=every)
    dev = pu.make(v, ages, policy=p)
    hd = dev.run(160)
    host = pu.make(v, ages)
    hh = pol.run_host_driven(host, p, 160)
    pu.assert_same_run(dev, host, hd, hh, planes=True)
    ora = pu.make(v, ages, factory=par_engine_factory)
    ho = pol.run_host_driven(ora, p, 160)
    pu.assert_same_run(dev, ora, hd, ho, planes=False)
    d0 = p.start_day(v['start_date'])
    assert list(dev.policy_levels) == [0] * d0 + [1] * (160 - d0) and d0 <= 102


def test_a_level_of_masks_alone():
    v, p = pu.hus_variables(), pu.masks_policy()
    dev = pu.make(v, policy=p)
    hd = dev.run(pu.HUS_DAYS)
    host = pu.make(v)
    hh = pol.run_host_driven(host, p, pu.HUS_DAYS)
    pu.assert_same_run(dev, host, hd, hh, planes=True)
    assert set(dev.policy_levels) == {0, 1}
    plain = pu.make(v).run(pu.HUS_DAYS)
    assert not np.array_equal(plain, hd)


# ---------------------------------------------------------------------------------------------- 10. beside the plain paths

def test_never_triggered_is_the_plain_run():
    v = pu.hus_variables()
    dev = pu.make(v, policy=pu.never_policy())
    hd = dev.run(200)
    plain = pu.make(v)
    hp = plain.run(200)
    _same_history(hd, hp)
    assert not dev.policy_levels.any() and list(dev.mobility_history) == list(plain.mobility_history)
    from filter_util import assert_same_day_state
    assert_same_day_state(dev, plain)


def test_plain_run_after_a_policy_run():
    """day 80 of the ward policy's year: level 2 in force; the plain days that follow keep its tables until the next dated
    change (the host-side mirrors of the tables follow the member's final level)"""
    v, p = pu.hus_variables(), pu.ward_policy()
    dev = pu.make(v, policy=p)
    h1 = dev.run(80)
    assert dev.policy_levels[-1] == 2
    dev.policy = None
    h2 = dev.run(60)
    host = pu.make(v)
    g1 = pol.run_host_driven(host, p, 80)
    g2 = host.run(60)
    _same_history(h1, g1)
    _same_history(h2, g2)
    from filter_util import assert_same_day_state
    assert_same_day_state(dev, host)
    # ... and a policy run in stretches is the run in one piece
    a, b = pu.make(v, policy=p), pu.make(v, policy=p)
    ha = np.concatenate([a.run(50), a.run(33), a.run(67)])
    hb = b.run(150)
    _same_history(ha, hb)
    assert_same_day_state(a, b)


# ---------------------------------------------------------------------------------------------- 11. branches

def test_branches_react_to_their_own_course():
    v, p = pu.hus_variables(), pu.ward_policy()
    past = pu.make(v, seed=3)
    past.run(pu.BRANCH_DAY)
    snap = past.snapshot()
    del past
    hist, ctxs = ensemble.run_branches(snap, v, pu.BRANCH_SEEDS, pu.BRANCH_DAYS, policy=p)
    for m, sd in enumerate(pu.BRANCH_SEEDS):
        ref = pu.make(v, seed=sd, snapshot=snap, ipc=None)
        hr = pol.run_host_driven(ref, p, pu.BRANCH_DAYS)
        pu.assert_same_run(ctxs[m], ref, hist[m], hr, planes=True)
    assert ctxs[0].policy_levels.max() >= 1


# ---------------------------------------------------------------------------------------------- the C ABI's refusals

def test_abi_refusals():
    v, ages = pu.mini_scenario()
    ctx = pu.make(v, ages)
    f = ctx.engine.policy_f
    good = pu.ward_policy().rule_abi(v['start_date'])

    def create(rule):
        h = ctypes.c_void_p()
        rc = f['policy_create'](ctx.engine._h, ctypes.byref(rule), ctypes.byref(h))
        return rc, h

    for field, value in (('n_levels', 1), ('n_levels', 9), ('signal', eng.C_NR), ('kind', 2), ('review_every', 0)):
        r = pu.ward_policy().rule_abi(v['start_date'])
        setattr(r, field, value)
        rc, _ = create(r)
        assert rc == -1 and b'policy' in ctx.engine.f['last_error'](), field
    r = pu.ward_policy().rule_abi(v['start_date'])
    r.up[1] = r.up[0] - 1
    assert create(r)[0] == -1
    r = pu.ward_policy().rule_abi(v['start_date'])
    r.down[0] = r.up[0] + 1
    assert create(r)[0] == -1
    rc, h = create(good)
    assert rc == 0
    # a bank level that was never uploaded
    plan = pu.make(v, ages).make_plan(2)
    _, arr, n = plan['segments'][0]
    assert f['policy_run_days'](h, arr, n, None, ctx.engine.alloc.stream()) == -1
    assert b'never uploaded' in ctx.engine.f['last_error']()
    assert f['group_policy_run_days'](h, arr, n, None, ctx.engine.alloc.stream()) == -1
    f['policy_destroy'](h)
