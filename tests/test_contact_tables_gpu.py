"""k_day's table searches and the host derivation that feeds them (csrc/reina_hip.hip: derive_contact_tables; csrc/k_contacts.inc:
contact_entry, the place groups, the count search) against oracle B on ADVERSARIAL contact tables (tests/table_util.py).

Oracle B copies the caller's tables as they are and searches them the plain way -- a linear `r < thr[j]` scan for the entry,
rc_count_from_draw for the count -- so both engines get the same transformed tables through the public upload and whole days
are compared bit for bit: history, counters, hot words, links, infectee chains, queues, bit planes (_run_and_compare of
tests/test_parity_gpu.py).  Every case asserts, on the very arrays its engines were given, the structural property that puts
it on its intended path; tests/test_contact_tables.py holds oracle B alone to the conditions that make the comparison mean
something (contacts drawn, infections, agents with symptoms) for exactly these populations, days and seeds.  No tolerance
anywhere: everything compared is integer or raw float bits.

No case provokes a fault: every table keeps its thresholds non-decreasing, its places below 6 and its age ranges inside the
ages (table_util.check_preconditions, asserted on every upload)."""
import ctypes

import numpy as np
import pytest

import table_util as tu
from reina_model_amd import engine as eng
from reina_model_amd import simulation
from test_parity_gpu import _assert_state_equal, _run_and_compare, _sharded_pair

pytestmark = pytest.mark.gpu


def _on_its_path(kind, seen):
    """the property of the uploaded tables that decides which path of the derivation and of k_day the case runs (the library's
    own flags are not readable through the ABI): asserted on every table either engine was given"""
    assert len(seen) >= 8, 'two engines, construction and three dated rebuilds each'
    for packed, A in seen:
        tu.check_preconditions(packed, A)
        d = tu.describe(packed, A)
        if kind == 'shuffled':          # grouped = 0 by derivation, !uniform_meta, rows staged in LDS
            assert d['place_runs'] > 6 and not d['uniform'] and d['rows'] <= tu.LDS_ROWS
        elif kind == 'ragged':          # counts 1 .. 96, grouped = 1 with G[6] < 6, !uniform_meta, rows staged in LDS
            assert d['counts'] == set(tu.RAGGED_COUNTS) and d['place_runs'] <= 6 and d['min_places'] < 6
            assert not d['uniform'] and d['rows'] <= tu.LDS_ROWS
            assert any(packed[2][a, 0] == 0 for a in range(A))
        elif kind == 'few_places':      # grouped = 1, G[6] in {1, 2, 5}
            assert d['place_runs'] == 5 and d['min_places'] == 1 and d['rows'] <= tu.LDS_ROWS
        elif kind == 'many_rows_uniform':   # 73 rows and 81 count rows through L2, uniform_meta = 1
            assert d['rows'] == 101 > tu.LDS_ROWS and d['nrc_patterns'] == 101 > tu.LDS_CROWS and d['uniform']
        elif kind == 'many_rows_mixed':     # ... with !uniform_meta, unsorted places, counts 2 .. 96 on either side of the edge
            assert d['rows'] == 101 > tu.LDS_ROWS and d['nrc_patterns'] == 101 > tu.LDS_CROWS
            assert not d['uniform'] and d['place_runs'] > 6
            assert set(packed[1][tu.LDS_ROWS:A].tolist()) == set(packed[1][:tu.LDS_ROWS].tolist()) == set(tu.RAGGED_COUNTS[1:])
        elif kind == 'clustered':       # 60 steps from the guide entry; uniform_meta = 1, grouped = 1
            assert d['max_in_one_top_byte'] >= 60 and d['uniform'] and d['place_runs'] == 6
        elif kind == 'count_extremes':  # count rows without contacts, of thousands of them; empty rows; more than LDS holds
            nrc, count = packed[0], packed[1]
            assert d['counts'] == {0, 90} and d['nrc_patterns'] > tu.LDS_CROWS
            assert (nrc[:A] <= 0).sum() >= 4 and (nrc[:A] >= 3000).sum() >= 2 and ((nrc[:A] > 0) & (nrc[:A] < 1)).sum() >= 2
            assert all(count[a] > 0 or not nrc[a] > 0 for a in range(A))
        else:
            raise AssertionError(kind)


CASES = [(k, {}) for k in tu.KINDS] + [
    ('many_rows_mixed', {'REINA_DAY_MODE': 'dense'}),
    ('many_rows_mixed', {'REINA_DAY_MODE': 'sparse'}),
    ('count_extremes', {'REINA_COUNT_ROW_CACHE': '0'}),
    ('ragged', {'REINA_COUNT_ROW_CACHE': '0'}),
]


@pytest.mark.parametrize('kind,env', CASES, ids=['-'.join([k] + ['%s=%s' % kv for kv in e.items()]) for k, e in CASES])
def test_whole_days_on_adversarial_tables_equal_oracle_b(kind, env, monkeypatch):
    """20 000 agents, 60 days of the default scenario (tables derived and uploaded at construction and at the dated mobility
    changes of days 23, 26 and 43, every time on transformed input) on the HIP engine and on oracle B"""
    for k, x in env.items():
        monkeypatch.setenv(k, x)
    seen = tu.install(monkeypatch, kind)
    v, ages = tu.scenario()
    _run_and_compare(v, ages, tu.SEED, tu.DAYS)
    _on_its_path(kind, seen)


def test_an_engine_group_on_more_rows_than_lds_holds_equals_its_members_alone(monkeypatch):
    """four seeds as one engine group (one launch per phase, group_lds_rows / group_lds_crows with 101 rows of each kind) ==
    the same seeds as single engines on oracle B: histories and final states"""
    import par_backend
    from reina_model_amd import ensemble
    seen = tu.install(monkeypatch, tu.GROUP_KIND)
    v, ages = tu.scenario()
    planner = simulation.make_context(v, age_counts=ages, seed=0)
    plan = planner.make_plan(tu.DAYS)
    members = [simulation.make_context(v, age_counts=ages, seed=s) for s in tu.GROUP_SEEDS]
    hist = ensemble.run_group_plan(members, plan)
    assert hist.shape == (len(tu.GROUP_SEEDS), tu.DAYS, eng.COUNTER_WORDS)
    for m, s in enumerate(tu.GROUP_SEEDS):
        cpu = simulation.make_context(v, age_counts=ages, seed=s, engine_factory=par_backend.par_engine_factory)
        assert np.array_equal(hist[m], cpu.run(tu.DAYS)), 'member %d (seed %d)' % (m, s)
        assert np.array_equal(members[m].engine.read_counters(), cpu.engine.read_counters())
        _assert_state_equal(members[m], cpu)
    _on_its_path(tu.GROUP_KIND, seen)


@pytest.mark.parametrize('attribution', ['exact', 'mirror'])
def test_two_shards_on_more_rows_than_lds_holds(attribution, monkeypatch):
    """two in-process shards (the exact-attribution kernels are instantiations of their own) on many_rows_mixed == the same on
    oracle B"""
    from reina_model_amd import sharding
    seen = tu.install(monkeypatch, tu.SHARD_KIND)
    v, ages = tu.scenario()
    gpu, cpu = _sharded_pair(v, ages, tu.SHARD_SEED, tu.SHARDS, attribution)
    for d in range(tu.DAYS):
        sharding.step_shards_together(gpu)
        sharding.step_shards_together(cpu)
        if d % 20 == 19:
            for a, b in zip(gpu, cpu):
                assert np.array_equal(a.engine.read_counters(), b.engine.read_counters()), d
    for a, b in zip(gpu, cpu):
        _assert_state_equal(a, b)
    assert len(seen) >= 4 * tu.SHARDS
    _on_its_path(tu.SHARD_KIND, seen)


def test_refused_tables_leave_the_engine_as_it_was(monkeypatch):
    """Through the raw ABI: an entry count below 0 or above REINA_MAX_ENTRIES, more than REINA_MAX_RANGES ranges, and an empty
    row for an age with contacts (k_day would read entry 0 of it) are refused with REINA_E_INVALID and a text that says why;
    after each refusal a valid upload and five more days still equal oracle B."""
    import par_backend
    seen = tu.install(monkeypatch, None)
    v, ages = tu.scenario()
    gpu = simulation.make_context(v, age_counts=ages, seed=tu.SEED)
    cpu = simulation.make_context(v, age_counts=ages, seed=tu.SEED, engine_factory=par_backend.par_engine_factory)
    assert np.array_equal(gpu.run(25), cpu.run(25))
    nrc, count, thr, meta, ranges = seen[-1][0]
    mask = gpu._uploaded_mask
    e = gpu.engine

    def refused(count_, ranges_, n_ranges, text):
        t, _keep = eng.Engine._tables_abi(nrc, count_, thr, meta, mask, ranges_)
        t.n_ranges = n_ranges
        rc = e.f['upload_contact_tables'](e._h, ctypes.byref(t), e.alloc.stream())
        assert rc != 0
        assert text in e.f['last_error']().decode()

    def bad_count(a, c):
        out = count.copy()
        out[a] = c
        return out
    pad = list(ranges) + [ranges[-1]] * (eng.MAX_RANGES - len(ranges))
    for args in ((bad_count(40, -1), ranges, len(ranges), 'contact entries per age must be in [0, REINA_MAX_ENTRIES]'),
                 (bad_count(40, eng.MAX_ENTRIES + 1), ranges, len(ranges), 'contact entries per age must be in [0, REINA_MAX_ENTRIES]'),
                 (count, pad, eng.MAX_RANGES + 1, 'more than REINA_MAX_RANGES contact ranges'),
                 (bad_count(40, 0), ranges, len(ranges), 'age 40 has contacts (nr_contacts_by_age > 0) but no contact entries')):
        refused(*args)
        for ctx in (gpu, cpu):
            ctx._upload_tables()
        assert np.array_equal(gpu.run(5), cpu.run(5)), args[3]
    with pytest.raises(eng.EngineError, match='age 40 has contacts'):   # ... and oracle B refuses the last one alike
        cpu.engine.upload_contact_tables(nrc, bad_count(40, 0), thr, meta, mask, ranges)
    for ctx in (gpu, cpu):
        ctx._upload_tables()
    assert np.array_equal(gpu.run(5), cpu.run(5))
    assert np.array_equal(gpu.engine.read_counters(), cpu.engine.read_counters())
    _assert_state_equal(gpu, cpu)
