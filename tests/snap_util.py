"""Test-side helpers for the snapshot format: populations of any size, deterministic synthetic engine states by named
pattern, and writing / reading those states into an oracle-B engine (numpy arrays) or a HIP engine (torch tensors).

A synthetic state is NOT a state a simulation could reach: its hot words, infectee indices and queue words are garbage.  It
only ever goes through pack and unpack (the snapshot kernels copy record words without following them); never step a day
on one -- the day kernels would follow those indices out of bounds."""
import copy

import numpy as np

from reina_model_amd import engine as eng
from reina_model_amd import simulation, snapshot as snapmod
from reina_model_amd.variables import VARIABLE_DEFAULTS

TILE = 512
NR_AGES = 101
NONE = 0xFFFFFFFF
GARBAGE = 0xA5A5A5A5
PATTERNS = ('empty', 'full', 'random', 'edges', 'alternating')
# k_init's cold record: claim (2 words) ~0, infector -1, n_infected 0, onset 0.0, vacc_day -1, first_infectee -1, next_sibling -1
COLD_DEFAULT = np.array([NONE, NONE, NONE, 0, 0, NONE, NONE, NONE], dtype=np.uint32)
STATE_ARRAYS = ('hot', 'cold', 'infectees', 'counters', 'control', 'queue0', 'queue1', 'level1')


def population(n):
    """age counts of n agents over 101 ages: all in one age below 101 agents, spread evenly otherwise"""
    ages = np.zeros(NR_AGES, dtype=np.int64)
    if n < NR_AGES:
        ages[40] = n
    else:
        ages[:] = n // NR_AGES
        ages[:n % NR_AGES] += 1
    return ages


def variables():
    return copy.deepcopy(VARIABLE_DEFAULTS)


def make_context(n, engine_factory=None):
    """a fresh Context of n agents (the HIP engine unless engine_factory says otherwise)"""
    return simulation.make_context(variables(), age_counts=population(n), seed=1, engine_factory=engine_factory)


def n_tiles(n):
    return (n + TILE - 1) // TILE


def recorded_agents(n, pattern, rng, p=0.3):
    """bool[n]: the agents whose hot word is non-zero"""
    if pattern == 'empty':
        return np.zeros(n, dtype=bool)
    if pattern == 'full':
        return np.ones(n, dtype=bool)
    if pattern == 'random':
        return rng.random(n) < p
    if pattern == 'edges':
        at = {0, 63, 64, 511, 512, n - 1}
        for t in range(1, n_tiles(n)):
            at |= {t * TILE - 1, t * TILE}
        rec = np.zeros(n, dtype=bool)
        rec[[i for i in at if 0 <= i < n]] = True
        return rec
    if pattern == 'alternating':
        return (np.arange(n) // TILE) % 2 == 0
    raise ValueError(pattern)


def synthetic_state(n, max_queue, pattern, seed=0, queues=False, p=0.3):
    """A deterministic engine state of n agents as uint32 arrays (STATE_ARRAYS).  Recorded agents (the pattern) have a random
    non-zero hot word and 0-8 inline slots filled in rank order (all 8 for 'full'); every cold word and every slot of the
    agents WITHOUT a record is random garbage, which a snapshot drops.  queues: lengths (max_queue, 1, 3) with random queue
    words, else (0, 0, 0); the control block holds them, its other words and the counters are random."""
    rng = np.random.default_rng([n, PATTERNS.index(pattern), seed, int(queues)])
    word = lambda *shape: rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)
    rec = recorded_agents(n, pattern, rng, p)
    hot = rng.integers(1, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    hot[~rec] = 0
    cold = word(n, eng.COLD_WORDS)
    inf = word(n, eng.INLINE_INFECTEES)
    used = np.full(n, eng.INLINE_INFECTEES) if pattern == 'full' else rng.integers(0, eng.INLINE_INFECTEES + 1, size=n)
    filled = np.arange(eng.INLINE_INFECTEES)[None, :] < used[:, None]
    slots = np.where(filled, inf, NONE)
    slots[filled & (slots == NONE)] = 0   # (a used slot holds an agent index: never ~0)
    inf = np.where(rec[:, None], slots, inf)
    qlen = (max_queue, 1, 3) if queues else (0, 0, 0)
    control = word(eng.L_NR)
    control[snapmod.L_QUEUE0:snapmod.L_QUEUE0 + 3] = qlen
    return dict(hot=hot, cold=cold, infectees=inf, counters=word(eng.COUNTER_WORDS), control=control,
                queue0=word(max_queue), queue1=word(max_queue), level1=word(max_queue), qlen=qlen)


def canonical(st, n):
    """what a restore of st's image leaves: k_init's words for agents with hot = 0, claims ~0, slots ~0 unless slot 0 is used,
    both bit planes rebuilt from hot (plane words past the last tile 0); the queues up to their lengths"""
    hot, rec = st['hot'], st['hot'] != 0
    cold = np.tile(COLD_DEFAULT, (n, 1))
    cold[rec, 2:] = st['cold'][rec, 2:]
    inf = np.full((n, eng.INLINE_INFECTEES), NONE, dtype=np.uint32)
    has = rec & (st['infectees'][:, 0] != NONE)
    inf[has] = st['infectees'][has]
    out = dict(hot=hot.copy(), cold=cold, infectees=inf, counters=st['counters'].copy(), control=st['control'].copy())
    for k, q in enumerate(('queue0', 'queue1', 'level1')):
        out[q] = st[q][:st['qlen'][k]].copy()
    for name, bit in (('active_bits', (hot & 0x8000) != 0), ('infected_bits', (hot & 7) != 0)):
        plane = np.zeros(eng.bits_words(n), dtype=np.uint32)
        packed = np.packbits(bit, bitorder='little')
        plane.view(np.uint8)[:len(packed)] = packed
        out[name] = plane
    return out


def _is_torch(engine):
    return not isinstance(engine.tensors['hot'], np.ndarray)


def write_state(engine, st):
    """copy st into an engine's arrays (oracle B: numpy; HIP: device tensors, synchronised before returning)"""
    for name in STATE_ARRAYS:
        src = np.ascontiguousarray(st[name]).reshape(-1)
        dst = engine.tensors[name]
        assert tuple(dst.shape) == (src.size,), name
        if _is_torch(engine):
            import torch
            dst.copy_(torch.from_numpy(src.view(np.int32)))
        else:
            dst.view(np.uint32)[:] = src
    if _is_torch(engine):
        engine.alloc.torch.cuda.synchronize()


def fill_garbage(engine):
    """GARBAGE into every per-agent word, the dense blocks, the queues and the bit-plane words of the tiles [0, 16 T); the
    plane words past them (the padding tile) 0, as reina_init_state leaves them"""
    n = engine.config.n_agents
    T16 = 16 * n_tiles(n)
    g = int(np.array(GARBAGE, dtype=np.uint32).view(np.int32))
    for name in STATE_ARRAYS + ('active_bits', 'infected_bits'):
        t = engine.tensors[name]
        if _is_torch(engine):
            t.fill_(g)
            if name.endswith('_bits'):
                t[T16:].zero_()
        else:
            np.asarray(t).view(np.uint32)[:] = GARBAGE
            if name.endswith('_bits'):
                t[T16:] = 0
    if _is_torch(engine):
        engine.alloc.torch.cuda.synchronize()


def read_state(engine):
    """the engine's persistent arrays as uint32 numpy arrays (cold and infectees as [n, 8])"""
    n = engine.config.n_agents
    out = {}
    for name in STATE_ARRAYS + ('active_bits', 'infected_bits'):
        t = engine.tensors[name]
        a = t.cpu().numpy() if _is_torch(engine) else np.array(t)
        a = np.ascontiguousarray(a).view(np.uint32)
        if name in ('cold', 'infectees'):
            a = a.reshape(n, -1)
        out[name] = a
    return out


def assert_state_equals(got, want, qlen):
    """got (read_state) against want (canonical): every word of the per-agent arrays, dense blocks and bit planes; the
    queues up to their lengths"""
    for name in ('hot', 'cold', 'infectees', 'counters', 'control', 'active_bits', 'infected_bits'):
        a, b = got[name], want[name]
        assert a.shape == b.shape, name
        bad = np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))
        assert len(bad) == 0, '%s: %d rows differ, first %d: %s != %s' % (name, len(bad), bad[0], a[bad[0]], b[bad[0]])
    for k, q in enumerate(('queue0', 'queue1', 'level1')):
        assert np.array_equal(got[q][:qlen[k]], want[q][:qlen[k]]), q


def group_geometry(n_tiles, members, n_cus):
    """(chunks, members per chunk, members of the last chunk) of reina_group_snap_unpack's launch (k_snapshot.inc): the
    members split over blockIdx.y when the tiles alone cannot fill the chip"""
    chunks = min(max(-(-4 * n_cus // n_tiles), 1), members)
    per = -(-members // chunks)
    chunks = -(-members // per)
    return chunks, per, members - (chunks - 1) * per
