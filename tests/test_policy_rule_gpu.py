"""k_policy's rule and table switch on driven signals (include/reina_policy.h).  The signal is not what an epidemic happens to
produce: it is written into a counter row before every call -- of idle populations, which keep the row as written, for the
rule (tests/policy_util.py: RULE_CASES), and into the `vaccinated` row of a live run of the mini scenario, which never
touches it, for the table switch (SWITCH_CASE).  The trace is compared word for word with policy_util.walk_rule, the plain
restatement of the rule; tests/test_policy.py holds the walker to step_numpy, asserts that these inputs take every branch,
and shows on oracle B that the rows stay as written.  Here every run asserts the latter from the history it gets back."""
import ctypes

import numpy as np
import pytest

import policy_util as pu
from par_backend import par_engine_factory
from reina_model_amd import engine as eng
from reina_model_amd import policy as pol

pytestmark = pytest.mark.gpu


def _assert_run_is_the_walk(run):
    case = run.case
    lo, hi = pu.signal_range(case.policy)
    assert run.trace.shape == (case.members, case.total, pol.TRACE_WORDS)
    unseen = np.setdiff1d(np.arange(case.total), case.days)
    for m in range(case.members):
        bad = np.argwhere(run.trace[m] != case.trace(m))
        assert len(bad) == 0, '%s member %d: %d trace words differ, first on day %d: (level, x) = %s, the rule gives %s' % (
            case.name, m, len(bad), bad[0][0], run.trace[m][bad[0][0]], case.trace(m)[bad[0][0]])
        assert not run.trace[m][unseen].any(), 'trace words of days the policy never saw'
        assert np.array_equal(run.history[m][:, lo:hi], case.written(m)), 'member %d: the signal row did not stay as written' % m


# ---------------------------------------------------------------------------------------------- the rule

@pytest.mark.parametrize('case', pu.RULE_CASES, ids=lambda c: c.name)
def test_rule_per_member_of_a_group(case):
    run = pu.DrivenDeviceRun(case)
    try:
        _assert_run_is_the_walk(run)
        # (the layout [member][REINA_MAX_DAYS][2]: the members stand at different levels)
        assert max(len(set(run.trace[:, d, 0])) for d in case.days) >= 2
    finally:
        run.close()


@pytest.mark.parametrize('name', pu.SINGLE_RULE_CASES)
def test_rule_for_one_engine(name):
    case = next(c for c in pu.RULE_CASES if c.name == name)
    for m in (0, 2):
        run = pu.DrivenDeviceRun(case.one(m), group=False)
        try:
            _assert_run_is_the_walk(run)
        finally:
            run.close()


def test_trace_read_back_on_ranges():
    case = next(c for c in pu.RULE_CASES if c.name == 'eight-increment-7')
    during = []

    def mid_run(run, lo, hi, seen):
        if seen and lo >= 60 and not during:      # a range that does not end on the last day run, while the run goes on
            during.append((lo - 12, run.dev.read_trace(lo - 12, 9)))

    run = pu.DrivenDeviceRun(case, before_call=mid_run)
    try:
        _assert_run_is_the_walk(run)
        whole = run.trace
        first, got = during[0]
        assert np.array_equal(got, np.stack([case.trace(m)[first:first + 9] for m in range(case.members)]))
        for first, n in ((40, 25), (57, 1), (0, 1), (10, case.total - 20), (case.total - 1, 1), (case.total, 0)):
            got = run.dev.read_trace(first, n)
            assert got.shape == (case.members, n, pol.TRACE_WORDS)
            assert np.array_equal(got, whole[:, first:first + n]), (first, n)
        assert len({tuple(whole[m, 57]) for m in range(case.members)}) >= 3
    finally:
        run.close()


# ---------------------------------------------------------------------------------------------- the table switch

@pytest.fixture(scope='module')
def solo():
    """member m of SWITCH_CASE on the device route, one engine: Context.run in stretches (made once per member)"""
    made = {}

    def get(m):
        if m not in made:
            ctx = pu.make_driven(pu.SWITCH_CASE, m, policy=pu.SWITCH_CASE.policy)
            made[m] = (ctx, pu.run_driven_context(ctx, pu.SWITCH_CASE, m, policy_on_context=True))
        return made[m]

    yield get
    made.clear()


def test_switch_case_device_equals_host_driven_equals_oracle(solo):
    case = pu.SWITCH_CASE
    dev, hd = solo(0)
    lo, hi = pu.signal_range(case.policy)
    assert np.array_equal(hd[:, lo:hi], case.written(0)), 'the live run touched the vaccinated row'
    assert np.array_equal(dev.policy_levels, case.levels(0))
    host = pu.make_driven(case, 0)
    hh = pu.run_driven_context(host, case, 0)
    pu.assert_same_run(dev, host, hd, hh, planes=True)
    ora = pu.make_driven(case, 0, factory=par_engine_factory)
    ho = pu.run_driven_context(ora, case, 0)
    pu.assert_same_run(dev, ora, hd, ho, planes=False)
    plain = pu.make_driven(case, 0).run(case.total)
    assert not np.array_equal(np.delete(plain, np.s_[lo:hi], axis=1), np.delete(hd, np.s_[lo:hi], axis=1))


def test_switch_case_group_members_against_single_engines(solo):
    from filter_util import assert_same_day_state
    case = pu.SWITCH_CASE
    run = pu.DrivenDeviceRun(case)
    try:
        _assert_run_is_the_walk(run)
        for m in range(case.members):
            one, hs = solo(m)
            bad = np.argwhere(run.history[m] != hs)
            assert len(bad) == 0, 'member %d: %d history words differ, first at (day, word) %s' % (m, len(bad), bad[0])
            assert np.array_equal(run.ctxs[m].policy_levels, one.policy_levels), 'member %d levels' % m
            assert list(run.ctxs[m].mobility_history) == list(one.mobility_history), 'member %d mobility factors' % m
            assert_same_day_state(run.ctxs[m], one)
    finally:
        run.close()


# ---------------------------------------------------------------------------------------------- the C ABI's refusals

def _refused(e, rc, *words):
    msg = e.f['last_error']()
    assert rc == -1 and b'policy' in msg and all(w in msg for w in words), (rc, msg)


@pytest.mark.parametrize('group', [False, True], ids=['one-engine', 'group'])
def test_abi_refusals_leave_the_run_as_it_was(group):
    case = next(c for c in pu.RULE_CASES if c.name == 'eight-level-equal-ups')
    case = case if group else case.one(1)
    done = []

    def refusals(run, lo, hi, seen):
        if not seen or lo < 30 or done:
            return
        done.append(lo)
        e = run.ctxs[0].engine
        f, stream = e.policy_f, e.alloc.stream()
        owner = run.group._h if group else e._h
        create = f['group_policy_create' if group else 'policy_create']
        for field, value, word in (('n_days', 0, b'1..28'), ('n_days', 29, b'1..28'), ('start_day', eng.MAX_DAYS, b'start_day'),
                                   ('start_day', 2 ** 32 - 1, b'start_day')):
            r = pol.Policy(pol.Signal('in_ward', 'increment', 7), pu.ladder(2), up=[5], down=[1]).rule_abi(pu.START_DATE)
            setattr(r, field, value)
            h = ctypes.c_void_p()
            _refused(e, create(owner, ctypes.byref(r), ctypes.byref(h)), word)
            assert not h.value
        h = run.dev._h
        t, _keep = eng.Engine._tables_abi(*run.plan['policy_banks'][0][0][0])
        _refused(e, f['policy_upload_level'](h, case.policy.n_levels, ctypes.byref(t), stream), b'level')
        out = np.zeros((case.members, 2, pol.TRACE_WORDS), dtype=np.int32)
        _refused(e, f['policy_read_trace'](h, eng.MAX_DAYS - 1, 2, out.ctypes.data, stream), b'trace range')
        _refused(e, f['policy_read_trace'](h, 0, 2, None, stream), b'out_host')
        assert not out.any()
        # a day beyond the trace, behind a good one: the call is refused as a whole, the good day does not run
        days = (eng.Day * 2)(run.day_list[lo], run.day_list[lo])
        days[1].day = eng.MAX_DAYS
        if group:
            rc = f['group_policy_run_days'](h, days, 2, None, stream)
        else:
            rc = f['policy_run_days'](h, days, 2, None, stream)
        _refused(e, rc, b'day >= REINA_MAX_DAYS')

    run = pu.DrivenDeviceRun(case, group=group, before_call=refusals)
    try:
        assert done
        _assert_run_is_the_walk(run)
    finally:
        run.close()
