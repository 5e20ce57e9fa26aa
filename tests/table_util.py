"""Adversarial contact tables for the day kernel's table searches (tests/test_contact_tables*.py).

Every table the product uploads comes from the one bundled contact file: 90 entries an age, six place runs in every row, the
same meta row for every age, some fifteen distinct rows.  The transforms here turn such a packed table
`(nrc, count, thr, meta, ranges)` (reina_model_amd.model.pack_contact_tables) into one that enters the other paths of
derive_contact_tables (csrc/reina_hip.hip) and of k_day's searches (csrc/k_contacts.inc): non-uniform meta, entry counts from
1 to REINA_MAX_ENTRIES, unsorted places, rows with fewer than six places, zero-width entries at the places' boundaries, more
distinct rows and count rows than the LDS image holds, long walks past the guide, count rows without contacts and with a
hundred of them.

`install(monkeypatch, kind)` wraps model.pack_contact_tables: Context._packed_tables looks the name up when it is called, so
the HIP Context and the oracle-B Context of a test get the same transformed arrays at construction, at every dated rebuild, in
a plan's segments, in a policy's banks and at a restore (all of them call Context._packed_tables).

The transforms work on INTEGER widths: w[j] = thr[j] - thr[j - 1], the last used entry closing at 2^32.  They change
(w, meta) and rebuild thr = min(cumsum(w), 0xFFFFFFFF), padded with 0xFFFFFFFF: thresholds stay non-decreasing (the ABI's
precondition), every row keeps an entry of non-zero width, every meta word keeps its place below 6 and its age range.
Everything is seeded by the row's class (its rank among the distinct rows of the input) or by the age: reproducible, and the
same for both engines.  `describe` says, from the arrays alone, what a table implies for the library's derivation -- the
library's own flags are not readable through the ABI, so the tests assert these on their inputs."""
import numpy as np

from reina_model_amd import engine as eng
from reina_model_amd import model

E = eng.MAX_ENTRIES
FULL = 1 << 32
NEVER = 0xFFFFFFFF
LDS_ROWS = 28    # REINA_LDS_ROWS: distinct contact rows in k_day's LDS image
LDS_CROWS = 20   # REINA_LDS_CROWS: distinct count rows in it
RAGGED_COUNTS = (1, 2, 3, 7, 45, 89, 90, 96)
RAGGED_SHIFT = 4   # class k gets RAGGED_COUNTS[(k + 4) % 8]: of the eight assignments the one with the liveliest epidemic on oracle B
KINDS = ('shuffled', 'ragged', 'few_places', 'many_rows_uniform', 'many_rows_mixed', 'clustered', 'count_extremes')
COUNT_BLOCKS = (0, 88)   # count_extremes: the first ages of the two blocks of extreme values (count_extreme_nrc)

_ORIGINAL_PACK = model.pack_contact_tables


# ---------------------------------------------------------------------------------------------- widths and thresholds
def widths(thr_row, c):
    """integer widths of a row's `c` used entries; the last one closes at 2^32"""
    t = np.asarray(thr_row[:c]).astype(np.int64)
    t[c - 1] = FULL
    return np.diff(np.concatenate([[0], t]))


def thresholds(w):
    """the padded threshold row of integer widths `w`"""
    out = np.full(E, NEVER, dtype=np.uint32)
    out[:len(w)] = np.minimum(np.cumsum(np.asarray(w, dtype=np.int64)), NEVER).astype(np.uint32)
    return out


def mass_by_key(w, m):
    """sum of widths per meta word = per (place, cmin, cmax, range_id)"""
    out = {}
    for wi, mi in zip(np.asarray(w).tolist(), np.asarray(m).tolist()):
        out[mi] = out.get(mi, 0) + wi
    return {k: v for k, v in out.items() if v}


def place_runs(m):
    pl = np.asarray(m).astype(np.int64) & 0xFF
    return 0 if len(pl) == 0 else 1 + int((np.diff(pl) != 0).sum())


def _row_key(count, thr, meta, a):
    c = int(count[a])
    return (c, thr[a, :c].tobytes(), meta[a, :c].tobytes())


def row_classes(count, thr, meta, A):
    """class of every age: the rank of its row among the distinct rows, in order of first appearance (as the library numbers them)"""
    seen, out = {}, []
    for a in range(A):
        out.append(seen.setdefault(_row_key(count, thr, meta, a), len(seen)))
    return out


def describe(packed, A):
    """what a packed table implies for derive_contact_tables, from the arrays alone"""
    nrc, count, thr, meta = packed[:4]
    keys = []
    for a in range(A):
        k = _row_key(count, thr, meta, a)
        if k not in keys:
            keys.append(k)
    c0 = keys[0][0]
    uniform = all(k[0] == c0 and k[2] == keys[0][2] for k in keys)
    runs = [place_runs(meta[a, :count[a]]) for a in range(A)]
    used = [a for a in range(A) if count[a] > 0]
    return dict(rows=len(keys),
                nrc_patterns=len(set(np.asarray(nrc[:A], dtype=np.float32).view(np.uint32).tolist())),
                uniform=uniform,
                place_runs=max(runs),
                min_place_runs=min(runs[a] for a in used),
                min_places=min(len(set((meta[a, :count[a]] & 0xFF).tolist())) for a in used),
                counts=set(int(c) for c in count[:A]),
                max_in_one_top_byte=max(int(np.bincount(thr[a, :count[a]] >> 24).max()) for a in used))


def check_preconditions(packed, A):
    """what every table passed to either engine must keep: counts in range, thresholds non-decreasing, an entry of non-zero
    width in every used row, places below 6, age ranges inside the ages, an empty row only without contacts"""
    nrc, count, thr, meta, ranges = packed
    for a in range(A):
        c = int(count[a])
        assert 0 <= c <= E
        if c == 0:
            assert not nrc[a] > 0
            continue
        t = thr[a, :c].astype(np.int64)
        assert np.all(np.diff(t) >= 0), a
        assert widths(thr[a], c).max() > 0 and widths(thr[a], c).min() >= 0
        m = meta[a, :c].astype(np.int64)
        assert np.all((m & 0xFF) < eng.NR_PLACES)
        assert np.all(((m >> 8) & 0xFF) <= ((m >> 16) & 0xFF)) and np.all(((m >> 16) & 0xFF) < A)
        assert np.all((m >> 24) < len(ranges))
        assert np.all(thr[a, c:] == NEVER)


# ---------------------------------------------------------------------------------------------- the pieces of the transforms
def resize_row(w, m, cc, rng):
    """a row of `cc` entries: tail entries merged into entry cc - 1 (shorter), or zero-width copies of entries chosen at random
    put right behind their originals (longer: the row stays sorted by place).  The padding conserves the mass of every key;
    the merge conserves the row's total and the keys of the entries in front of the merged one."""
    c = len(w)
    if cc < c:
        return np.concatenate([w[:cc - 1], [w[cc - 1:].sum()]]), m[:cc].copy()
    if cc > c:
        at = np.sort(rng.choice(c, size=cc - c, replace=False))
        w2, m2 = [], []
        for j in range(c):
            w2.append(w[j])
            m2.append(m[j])
            if j in at:
                w2.append(0)
                m2.append(m[j])
        return np.array(w2, dtype=np.int64), np.array(m2, dtype=np.uint32)
    return w.copy(), m.copy()


def zero_some(w, m, k, rng):
    """about a fifth of the widths zeroed, their mass moved to the first surviving entry (the row's total is conserved); by
    class k: k % 3 == 0 a zero-width FIRST entry (thr[0] == 0), k % 3 == 1 a zero-width run across the first place boundary,
    k % 3 == 2 the whole second place without mass"""
    c = len(w)
    w = w.copy()
    if c < 2:
        return w
    z = rng.random(c) < 0.2
    pl = m.astype(np.int64) & 0xFF
    bounds = np.flatnonzero(np.diff(pl) != 0) + 1   # first entries of the later places
    if k % 3 == 0:
        z[0] = True
    elif k % 3 == 1 and len(bounds):
        b = int(bounds[0])
        z[max(b - 2, 0):b + 2] = True
    elif k % 3 == 2 and len(bounds):
        b0 = int(bounds[0])
        b1 = int(bounds[1]) if len(bounds) > 1 else c
        z[b0:b1] = True
    z &= w > 0
    if z.all():
        z[int(np.argmax(w))] = False
    keep = int(np.flatnonzero(~z)[0])
    w[keep] += w[z].sum()
    w[z] = 0
    return w


def move_units(w, units):
    """`units` of width from the widest entry to its neighbour: rows that differ by age and by nothing a run could notice"""
    w = w.copy()
    if len(w) < 2:
        return w
    d = int(np.argmax(w))
    r = d + 1 if d + 1 < len(w) else d - 1
    w[d] -= units
    w[r] += units
    return w


FEW_PLACES_RUNS = {1: (2, 2, 2, 2, 2, 2), 2: (0, 0, 0, 3, 3, 3), 5: (0, 0, 2, 3, 4, 5)}


def few_places_row(w, m, k):
    """the row's six place runs mapped onto 1, 2 or 5 places (run r takes the place of run FEW_PLACES_RUNS[n][r]); for odd k
    the entries on either side of the first remaining boundary lose their width to their neighbours inside the place"""
    n = (1, 2, 5)[k % 3]
    pl = m.astype(np.int64) & 0xFF
    starts = np.concatenate([[0], np.flatnonzero(np.diff(pl) != 0) + 1])
    run_of = np.searchsorted(starts, np.arange(len(m)), side='right') - 1
    assert len(starts) == 6, 'the bundled contact file has six place runs a row'
    new_pl = np.array([pl[starts[FEW_PLACES_RUNS[n][r]]] for r in run_of], dtype=np.uint32)
    m2 = (m & np.uint32(0xFFFFFF00)) | new_pl
    w2 = w.copy()
    b = np.flatnonzero(np.diff(new_pl.astype(np.int64)) != 0) + 1
    if k % 2 == 1 and len(b) and b[0] >= 2 and b[0] + 1 < len(w2):
        j = int(b[0])
        w2[j - 2] += w2[j - 1]
        w2[j - 1] = 0
        w2[j + 1] += w2[j]
        w2[j] = 0
    return w2, m2


def clustered_row(w, m, k):
    """even k: 60 of the row's 90 entries inside the top byte 64 (width 2^24 / 64 each), ten entries in front sharing
    [0, 64 << 24), twenty behind sharing the rest: a draw with that top byte walks up to 60 steps from its guide entry.
    odd k: entries 20..49 of width 1, taken from the widest entry."""
    c = len(w)
    assert c == 90
    if k % 2 == 0:
        w2 = np.zeros(c, dtype=np.int64)
        head = 64 << 24
        w2[:10] = head // 10
        w2[0] += head - w2[:10].sum()
        w2[10:70] = (1 << 24) // 64
        rest = FULL - head - 60 * ((1 << 24) // 64)
        w2[70:] = rest // 20
        w2[70] += rest - w2[70:].sum()
        return w2
    w2 = w.copy()
    d = int(np.argmax(w2))
    for j in range(20, 50):
        if j != d:
            w2[d] -= 1 - w2[j]
            w2[j] = 1
    return w2


def _extreme_slot(a):
    for first in COUNT_BLOCKS:
        if first <= a < first + 8:
            return a - first
    return None


def count_extreme_nrc(a):
    """nr_contacts_by_age of age a.  The eight ages from each age of COUNT_BLOCKS on run through: a hundred contacts, 250, a
    value at which every count threshold is 0 (the guide byte 100), no contacts (0.0, a negative value), fewer than one, fewer
    than two, the usual dozen.  Every other age keeps the usual dozen -- with the extreme values on more ages the population
    is through the epidemic in three weeks.  All but 0.0 differ a little by age: more count rows than the LDS image holds,
    the first block's among the rows staged in LDS, the second block's among those read through L2."""
    q = _extreme_slot(a)
    if q is None:
        return 11.5 + 0.01 * a
    return (99.5 + 0.01 * a, 250.0 + 0.1 * a, 3000.0 + a, 0.0, -1.0 - a, 0.3 + 0.001 * a, 1.9 + 0.001 * a, 11.5 + 0.01 * a)[q]


def count_extreme_empty(a):
    """the ages without contacts that also get count = 0: the first block's 0.0, the second block's negative value"""
    return a in (COUNT_BLOCKS[0] + 3, COUNT_BLOCKS[1] + 4)


# ---------------------------------------------------------------------------------------------- the transforms
def transform(kind, packed, A):
    """the transformed copy of a packed table (the input is not touched: pack_contact_tables hands out cached arrays)"""
    nrc, count, thr, meta, ranges = packed
    nrc, count, thr, meta = (np.array(x, copy=True) for x in (nrc, count, thr, meta))
    cls = row_classes(count, thr, meta, A)
    kid = KINDS.index(kind)
    for a in range(A):
        c, k = int(count[a]), cls[a]
        w, m = widths(thr[a], c), meta[a, :c].copy()
        rk, ra = np.random.default_rng([2020, kid, k]), np.random.default_rng([2021, kid, a])
        if kind == 'shuffled':
            p = rk.permutation(c)
            w, m = w[p], m[p]
        elif kind == 'ragged':
            w, m = resize_row(w, m, RAGGED_COUNTS[(k + RAGGED_SHIFT) % 8], rk)
            w = zero_some(w, m, k, rk)
        elif kind == 'few_places':
            w, m = few_places_row(w, m, k)
        elif kind == 'many_rows_uniform':
            w = move_units(w, a + 1)
            nrc[a] = np.float32(nrc[a] * (1.0 + a * 2.0 ** -12))
        elif kind == 'many_rows_mixed':
            # ragged rows by AGE (every count but 1, which leaves nothing to tell rows apart by), their entries permuted by age
            w, m = resize_row(w, m, RAGGED_COUNTS[1 + a % 7], ra)
            w = zero_some(w, m, a, ra)
            p = ra.permutation(len(w))
            w, m = move_units(w[p], a + 1), m[p]
            nrc[a] = np.float32(nrc[a] * (1.0 + a * 2.0 ** -12))
        elif kind == 'clustered':
            w = clustered_row(w, m, k)
        elif kind == 'count_extremes':
            nrc[a] = np.float32(count_extreme_nrc(a))
            if count_extreme_empty(a):   # (no row at all)
                w, m = w[:0], m[:0]
        else:
            raise ValueError(kind)
        assert len(w) == 0 or (w.min() >= 0 and int(w.sum()) == FULL), (kind, a)
        thr[a] = thresholds(w)
        meta[a] = 0
        meta[a, :len(w)] = m
        count[a] = len(w)
    return nrc, count, thr, meta, ranges


def install(monkeypatch, kind):
    """model.pack_contact_tables -> its `kind` transform for the rest of the test; returns the list every transformed table
    is appended to, (packed, nr_ages) in upload order.  kind None: the tables as they are, recorded."""
    seen = []

    def pack(tables, nr_ages):
        out = _ORIGINAL_PACK(tables, nr_ages)
        if kind is not None:
            out = transform(kind, out, nr_ages)
        seen.append((out, nr_ages))
        return out
    monkeypatch.setattr(model, 'pack_contact_tables', pack)
    return seen


# ---------------------------------------------------------------------------------------------- the runs of the GPU cases
# tests/test_contact_tables_gpu.py runs exactly these; tests/test_contact_tables.py holds oracle B alone to the conditions the
# GPU cases rely on (contacts drawn, infections, agents with symptoms) for exactly these populations, days and seeds
N_AGENTS = 20000
SEED = 1
DAYS = 60
GROUP_KIND, GROUP_SEEDS = 'many_rows_mixed', (1, 2, 3, 4)
SHARD_KIND, SHARD_SEED, SHARDS = 'many_rows_mixed', 1, 2


def scenario():
    """the default scenario at the mini size: its dated limit-mobility interventions (days 23, 26 and 43) rebuild the tables
    mid-run, so every transform is derived and uploaded four times"""
    import copy
    from reina_model_amd import datasets
    from reina_model_amd.variables import VARIABLE_DEFAULTS
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    v.update(hospital_beds=12, icu_units=2)
    return v, datasets.scaled_population(N_AGENTS)


def sharded_contexts(v, ages, seed, attribution, engine_factory=None):
    """SHARDS in-process shards of one population (as tests/test_parity_gpu.py: _sharded_pair builds each side)"""
    from reina_model_amd import sharding, simulation
    members = []
    kw = {} if engine_factory is None else dict(engine_factory=engine_factory)
    return [simulation.make_context(v, age_counts=ages, seed=seed,
                                    comm=sharding.InProcessComm(r, SHARDS, members, attribution=attribution), **kw)
            for r in range(SHARDS)]
