"""The adversarial contact tables of tests/table_util.py, on the CPU: the transforms do what they claim (mass, structure,
preconditions), the specification both engines' searches implement holds on tables with ties, oracle B ALONE meets the
conditions tests/test_contact_tables_gpu.py relies on -- for exactly its populations, days and seeds --, and the oracle library
refuses an empty row for an age with contacts as the HIP library does."""
import ctypes

import numpy as np
import pytest

import par_backend
import table_util as tu
from reina_model_amd import engine as eng
from reina_model_amd import simulation

S0 = eng.C_NR * eng.MAX_AGES


def _total(h, name):
    k = eng.C_NAMES.index(name) * eng.MAX_AGES
    return np.asarray(h)[..., k:k + eng.MAX_AGES].sum(axis=-1)


@pytest.fixture(scope='module')
def base_tables():
    """the packed tables of the default scenario as the product uploads them over the GPU cases' days: at construction and
    at each dated rebuild"""
    mp = pytest.MonkeyPatch()
    try:
        seen = tu.install(mp, None)
        v, ages = tu.scenario()
        ctx = simulation.make_context(v, age_counts=ages, seed=tu.SEED, engine_factory=par_backend.par_engine_factory)
        ctx.run(tu.DAYS)
    finally:
        mp.undo()
    assert len(seen) >= 4, 'construction and the rebuilds of days 23, 26 and 43'
    return seen


def test_the_bundled_tables_are_what_the_transforms_assume(base_tables):
    """... and why the adversarial tier exists: none of the paths below is entered by the product's own tables"""
    for packed, A in base_tables:
        tu.check_preconditions(packed, A)
        d = tu.describe(packed, A)
        assert A == 101 and d['counts'] == {90} and d['uniform'] and d['place_runs'] == 6 and d['min_places'] == 6
        assert d['rows'] <= tu.LDS_ROWS and d['nrc_patterns'] <= tu.LDS_CROWS
        assert all(packed[2][a, 0] != 0 for a in range(A))


def _rows(packed, a):
    c = int(packed[1][a])
    return tu.widths(packed[2][a], c), packed[3][a, :c]


@pytest.mark.parametrize('kind', tu.KINDS)
def test_every_transform_keeps_the_preconditions_and_every_rows_mass(kind, base_tables):
    for packed, A in base_tables:
        out = tu.transform(kind, packed, A)
        tu.check_preconditions(out, A)
        assert out[4] is packed[4] or out[4] == packed[4]
        for a in range(A):
            if out[1][a]:
                w, _ = _rows(out, a)
                assert int(w.sum()) == tu.FULL
        again = tu.transform(kind, packed, A)   # reproducible: both engines of a test get the same arrays
        assert all(np.array_equal(x, y) for x, y in zip(out[:4], again[:4]))


def test_mass_per_place_and_age_range_is_conserved_where_claimed(base_tables):
    """integer widths per (place, cmin, cmax, range_id), per age: unchanged by `shuffled`; by many_rows_uniform up to the
    a + 1 units it moves between two neighbours; by the padding of `ragged`; the merge of `ragged` keeps the entries in front
    of the merged one and the total, its zeroing the total and every entry it neither zeroes nor feeds"""
    packed, A = base_tables[-1]
    sh, mu = tu.transform('shuffled', packed, A), tu.transform('many_rows_uniform', packed, A)
    for a in range(A):
        w, m = _rows(packed, a)
        base = tu.mass_by_key(w, m)
        ws, ms = _rows(sh, a)
        got = tu.mass_by_key(ws, ms)
        if got != base:
            # 2^32 is no threshold: where entries of width zero end up behind the one that closes the row, that one's
            # threshold saturates at 0xFFFFFFFF and the draw 0xFFFFFFFF goes to the last entry -- one unit, no more
            diff = {k: got.get(k, 0) - base.get(k, 0) for k in set(got) | set(base) if got.get(k, 0) != base.get(k, 0)}
            assert sorted(diff.values()) == [-1, 1] and diff[int(ms[-1])] == 1 and ws[-1] == 1, (a, diff)
        w2, m2 = _rows(mu, a)
        assert np.array_equal(m2, m)
        assert np.abs(w2 - w).sum() == 2 * (a + 1) and np.abs(w2 - w).max() == a + 1
        rng = np.random.default_rng([7, a])
        wp, mp_ = tu.resize_row(w, m, 96, rng)
        assert len(wp) == 96 and tu.mass_by_key(wp, mp_) == base and tu.place_runs(mp_) == 6
        for cc in (1, 2, 3, 7, 45, 89):
            wm, mm = tu.resize_row(w, m, cc, rng)
            assert len(wm) == cc and int(wm.sum()) == tu.FULL
            assert np.array_equal(wm[:cc - 1], w[:cc - 1]) and np.array_equal(mm, m[:cc])
        wz = tu.zero_some(w, m, a, rng)
        assert int(wz.sum()) == tu.FULL
        changed = np.flatnonzero(wz != w)
        fed = [j for j in changed if wz[j] > 0]
        assert len(fed) <= 1 and all(wz[j] == 0 for j in changed if j not in fed)
        newly = ((wz == 0) & (w > 0)).mean()   # a fifth at random, and at most a whole place (15 of 90) on top
        assert 0.08 < newly < 0.2 + 15 / 90 + 0.1


def test_the_structure_each_transform_promises(base_tables):
    """what places each GPU case on its intended path of derive_contact_tables and k_day (the GPU file asserts the same on
    the tables its engines were given)"""
    for packed, A in base_tables:
        d = {k: tu.describe(tu.transform(k, packed, A), A) for k in tu.KINDS}
        t = {k: tu.transform(k, packed, A) for k in ('ragged', 'few_places', 'clustered', 'count_extremes', 'many_rows_mixed')}
        # unsorted places (grouped = 0 by derivation), meta rows differ, every row in LDS
        assert d['shuffled']['place_runs'] > 6 and not d['shuffled']['uniform'] and d['shuffled']['rows'] <= tu.LDS_ROWS
        assert d['shuffled']['counts'] == {90}
        # every count, rows sorted by place (grouped stays 1) with fewer than six places among them, all in LDS
        r = d['ragged']
        assert r['counts'] == set(tu.RAGGED_COUNTS) and r['place_runs'] <= 6 and r['min_places'] == 1 and not r['uniform']
        assert r['rows'] <= tu.LDS_ROWS
        nrc, count, thr, meta, _ = t['ragged']
        first_zero = boundary_zero = empty_place = 0
        for a in range(A):
            c = int(count[a])
            w, m = tu.widths(thr[a], c), meta[a, :c]
            pl = m.astype(np.int64) & 0xFF
            first_zero += int(c > 1 and thr[a, 0] == 0)
            b = np.flatnonzero(np.diff(pl) != 0) + 1
            boundary_zero += int(any(w[j - 1] == 0 and w[j] == 0 for j in b))
            empty_place += int(any(w[pl == p].sum() == 0 for p in set(pl.tolist())))
        assert first_zero >= 5 and boundary_zero >= 5 and empty_place >= 1
        # 1, 2 and 5 places, sorted, zero-width entries on both sides of a boundary
        f = d['few_places']
        assert f['place_runs'] == 5 and f['min_places'] == 1 and f['counts'] == {90} and f['rows'] <= tu.LDS_ROWS
        nrc, count, thr, meta, _ = t['few_places']
        places = {len(set((meta[a, :90] & 0xFF).tolist())) for a in range(A)}
        assert places == {1, 2, 5}
        bz = 0
        for a in range(A):
            w, pl = tu.widths(thr[a], 90), meta[a, :90].astype(np.int64) & 0xFF
            assert tu.place_runs(meta[a, :90]) == len(set(pl.tolist()))   # sorted
            bz += int(any(w[j - 1] == 0 and w[j] == 0 for j in np.flatnonzero(np.diff(pl) != 0) + 1))
        assert bz >= 5
        # more rows and count rows than LDS holds: 101 - 28 rows and 101 - 20 count rows are read through L2
        for k in ('many_rows_uniform', 'many_rows_mixed'):
            assert d[k]['rows'] == 101 and d[k]['nrc_patterns'] == 101
        assert d['many_rows_uniform']['uniform'] and d['many_rows_uniform']['place_runs'] == 6
        m = d['many_rows_mixed']
        assert not m['uniform'] and m['place_runs'] > 6 and m['counts'] == set(tu.RAGGED_COUNTS[1:])
        # ... with every count on either side of the LDS image's edge
        cm = t['many_rows_mixed'][1]
        assert set(cm[:tu.LDS_ROWS].tolist()) == set(cm[tu.LDS_ROWS:101].tolist()) == set(tu.RAGGED_COUNTS[1:])
        # a walk of 60 steps past the guide (the bundled tables: 20-odd), a run of width-1 entries; sorted, uniform meta
        c = d['clustered']
        assert c['max_in_one_top_byte'] >= 60 and c['uniform'] and c['place_runs'] == 6
        thr = t['clustered'][2]
        assert any((np.diff(thr[a, :90].astype(np.int64)) == 1).sum() >= 29 for a in range(A))
        assert any(np.bincount(thr[a, :90] >> 24).max() >= 60 for a in range(A))
        # count rows: without contacts (with and without entries), below one, a hundred and more, every threshold 0
        nrc, count = t['count_extremes'][:2]
        assert d['count_extremes']['nrc_patterns'] > tu.LDS_CROWS and d['count_extremes']['counts'] == {0, 90}
        for a in range(A):
            assert count[a] > 0 or not nrc[a] > 0
        assert sum(1 for a in range(A) if count[a] == 0) == 2
        assert sum(1 for a in range(A) if not nrc[a] > 0 and count[a] > 0) == 2
        for lo, hi in ((0.0, 1.0), (1.0, 2.0), (99.0, 101.0), (249.0, 300.0), (2999.0, 4000.0)):
            hit = [a for a in range(A) if lo < nrc[a] < hi]
            assert any(a < 8 for a in hit) and any(a >= tu.COUNT_BLOCKS[1] for a in hit), (lo, hi)
        # (the distinct nrc values before the second block fill the LDS image's count rows: the block's are read through L2)
        assert len(set(nrc[:tu.COUNT_BLOCKS[1]].view(np.uint32).tolist())) > tu.LDS_CROWS


def test_a_count_row_of_thousands_of_contacts_has_every_threshold_zero():
    """the value count_extremes uses for "every threshold 0, guide byte 100" gives that (csrc/reina_contacts.h), 250 does not;
    no contacts: every threshold `never`"""
    L = par_backend.lib()
    L.par_test_count_from_draw.restype = ctypes.c_int
    L.par_test_count_from_draw.argtypes = [ctypes.c_float, ctypes.c_int, ctypes.c_uint32]
    assert L.par_test_count_from_draw(3000.0, 0, 0) == 100 and L.par_test_count_from_draw(3088.0, 0, 0) == 100
    assert L.par_test_count_from_draw(250.0, 0, 0) < 100
    for nrc in (0.0, -1.0, -89.0):
        assert L.par_test_count_from_draw(nrc, 0, 0xFFFFFFFE) == 0 and L.par_test_count_from_draw(nrc, 1, 0xFFFFFFFE) == 0


@pytest.mark.parametrize('kind', [k for k in tu.KINDS if k != 'count_extremes'])
def test_first_entry_above_the_draw_on_tables_with_ties(kind, base_tables):
    """The specification oracle B's scan implements (oracle/reina_par.c: run_contacts) and k_day's shortcuts have to
    reproduce: the first entry with r < thr, else the last.  Restated in numpy and held against np.searchsorted on every
    distinct row of the transformed tables, for every threshold, its two neighbours, 0 and 0xFFFFFFFE -- repeated thresholds
    (zero-width entries) at the front, in the middle and at the end included."""
    packed, A = base_tables[-1]
    nrc, count, thr, meta, _ = tu.transform(kind, packed, A)
    done = set()
    for a in range(A):
        c = int(count[a])
        key = (c, thr[a, :c].tobytes())
        if key in done:
            continue
        done.add(key)
        t = thr[a, :c].astype(np.int64)
        r = np.unique(np.clip(np.concatenate([t, t - 1, t + 1, [0, 0xFFFFFFFE]]), 0, 0xFFFFFFFE))
        below = r[:, None] < t[None, :]
        plain = np.where(below.any(axis=1), below.argmax(axis=1), c - 1)
        fast = np.minimum(np.searchsorted(t, r, side='right'), c - 1)
        assert np.array_equal(plain, fast), (kind, a)
        w = tu.widths(thr[a], c)
        # (an entry of width zero is selected by no draw -- except as "the last one" by draws at or above every threshold)
        picked = set(plain.tolist())
        assert all(w[j] > 0 or j == c - 1 for j in picked), (kind, a)


def _conditions(hist, what):
    """what a GPU case needs of its run for the comparison to mean something (hist: [days, COUNTER_WORDS], rows before each
    day; the run ended without the problem flag or it would have raised)"""
    hist = np.asarray(hist)
    assert hist[:, S0 + eng.S_PROBLEM].max() == 0, what
    contacts = int(hist[:, S0 + eng.S_DAILY_CONTACTS:S0 + eng.S_DAILY_CONTACTS + eng.NR_PLACES].sum())
    assert contacts >= 100_000, (what, contacts)
    infected = _total(hist, 'all_infected')
    assert infected[-1] >= 1000, (what, infected[-1])
    # agents with symptoms (the ill class of the count search: five comparisons): under the scenario's testing mode --
    # everyone with symptoms is tested, from day 2 -- a new detection is an agent who is ill with symptoms that day
    detected = _total(hist, 'all_detected')
    assert int((np.diff(detected) > 0).sum()) >= 10, what
    return contacts, int(infected[-1])


@pytest.mark.parametrize('kind', tu.KINDS)
def test_oracle_b_alone_meets_the_conditions_of_the_gpu_cases(kind, monkeypatch):
    """the single-engine case of every transform: population, seed and days of tests/test_contact_tables_gpu.py"""
    seen = tu.install(monkeypatch, kind)
    v, ages = tu.scenario()
    ctx = simulation.make_context(v, age_counts=ages, seed=tu.SEED, engine_factory=par_backend.par_engine_factory)
    hist = ctx.run(tu.DAYS)
    _conditions(hist, kind)
    assert len(seen) >= 4   # the tables were rebuilt mid-run on transformed input
    if kind == 'count_extremes':   # the extreme count rows are drawn from: agents of those ages were infectious
        infected = np.asarray(hist)[-1, eng.C_NAMES.index('all_infected') * eng.MAX_AGES:][:101]
        for first in tu.COUNT_BLOCKS:
            assert np.all(infected[first:first + 8] >= 5), infected[first:first + 8]


def test_oracle_b_alone_meets_the_conditions_of_the_group_and_shard_cases(monkeypatch):
    tu.install(monkeypatch, tu.GROUP_KIND)
    v, ages = tu.scenario()
    for seed in tu.GROUP_SEEDS:
        ctx = simulation.make_context(v, age_counts=ages, seed=seed, engine_factory=par_backend.par_engine_factory)
        _conditions(ctx.run(tu.DAYS), 'group seed %d' % seed)
    from reina_model_amd import sharding
    assert tu.SHARD_KIND == tu.GROUP_KIND
    for attribution in ('exact', 'mirror'):
        shards = tu.sharded_contexts(v, ages, tu.SHARD_SEED, attribution, engine_factory=par_backend.par_engine_factory)
        rows = []
        for _ in range(tu.DAYS):
            rows.append(sharding.reduce_counters(shards))
            sharding.step_shards_together(shards)
        _conditions(np.array(rows), 'two shards, ' + attribution)


def _raw_tables(packed, A, mask=None):
    nrc, count, thr, meta, ranges = packed
    mask = np.zeros((eng.MAX_AGES, 8), dtype=np.float32) if mask is None else mask
    return nrc, count, thr, meta, mask, ranges


def test_oracle_b_refuses_an_empty_row_for_an_age_with_contacts(base_tables):
    """count == 0 with nr_contacts_by_age > 0: run_contacts would index entry -1 of the row.  Refused with REINA_E_INVALID and a
    message naming the age, like the HIP library (tests/test_contact_tables_gpu.py); count == 0 without contacts stays legal"""
    packed, A = base_tables[0]
    v, ages = tu.scenario()
    ctx = simulation.make_context(v, age_counts=ages, seed=tu.SEED, engine_factory=par_backend.par_engine_factory)
    count = packed[1].copy()
    count[37] = 0
    with pytest.raises(eng.EngineError, match=r'age 37 has contacts .*no contact entries'):
        ctx.engine.upload_contact_tables(*_raw_tables((packed[0], count, packed[2], packed[3], packed[4]), A))
    nrc = packed[0].copy()
    for value in (0.0, -2.0, np.float32('nan')):
        nrc[37] = value
        ctx.engine.upload_contact_tables(*_raw_tables((nrc, count, packed[2], packed[3], packed[4]), A))
