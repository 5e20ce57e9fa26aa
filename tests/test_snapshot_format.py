"""The snapshot format on the CPU: a plain per-agent writer of the image, built from include/reina_snapshot.h and DESIGN.md
6b alone, against the numpy packer (snapshot.pack_numpy, the format's executable specification) on synthetic states at tile
edges; the numpy unpacker against the state they encode; the Python mirror of the C header against the header."""
import os
import re

import numpy as np
import pytest

import par_backend
import snap_util
from reina_model_amd import engine as eng
from reina_model_amd import snapshot as snapmod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 63, 64, 65, 511, 512, 513, 4099)


def _header_text(name):
    text = open(os.path.join(ROOT, 'include', name)).read()
    return re.sub(r'/\*.*?\*/', '', text, flags=re.S)


def header_constants():
    """name -> value of every valued #define and every enumerator of include/reina_snapshot.h"""
    text = _header_text('reina_snapshot.h')
    out = {}
    for name, value in re.findall(r'^#define\s+(REINA_\w+)\s+(0x[0-9A-Fa-f]+|\d+)u?\s*$', text, flags=re.M):
        out[name] = int(value, 0)
    for body in re.findall(r'\benum\s*\{(.*?)\}', text, flags=re.S):
        at = 0
        for item in (x.strip() for x in body.split(',')):
            if not item:
                continue
            m = re.fullmatch(r'(\w+)(?:\s*=\s*(\d+))?', item)
            assert m, item
            at = int(m.group(2)) if m.group(2) else at
            out[m.group(1)] = at
            at += 1
    return out


def _fnv1a64(data):
    h = 0xCBF29CE484222325
    for b in data:
        h = ((h ^ b) * 0x100000001B3) % (1 << 64)
    return h


def reference_image(config, disease, st, testing_ever):
    """The image of state st, one agent at a time, from the header's description of the layout (no snapshot.layout)."""
    c = header_constants()
    n, tile, rw = config.n_agents, c['REINA_SNAP_TILE'], c['REINA_SNAP_RECORD_WORDS']
    T = -(-n // tile)
    qlen = [int(x) for x in st['control'][2:5]]   # (REINA_L_QUEUE0, QUEUE1, LEVEL1)
    base, slots, tb, ts = [], [], [0], [0]
    for t in range(T):
        for i in range(t * tile, min(n, (t + 1) * tile)):
            h = int(st['hot'][i])
            if h == 0:
                continue
            has = int(st['infectees'][i][0]) != 0xFFFFFFFF
            base.append([i | (has << 31), h] + [int(w) for w in st['cold'][i][2:8]])
            if has:
                slots.append([int(w) for w in st['infectees'][i]])
        tb.append(len(base))
        ts.append(len(slots))
    words = [0] * c['REINA_SNAP_HEADER_WORDS']
    words += [int(w) for w in st['counters']] + [int(w) for w in st['control']] + tb + ts
    words += [0] * (-len(words) % 8)
    assert len(base) == 0 or len(words) % rw == 0
    for r in base + slots:
        words += r
    for k, q in enumerate(('queue0', 'queue1', 'level1')):
        words += [int(w) for w in st[q][:qlen[k]]]
    hd = {'MAGIC': c['REINA_SNAP_MAGIC'], 'VERSION': c['REINA_SNAPSHOT_VERSION'], 'N_AGENTS': n, 'NR_AGES': config.nr_ages,
          'NR_VARIANTS': config.nr_variants, 'N_TILES': T, 'N_BASE': len(base), 'N_SLOT': len(slots),
          'FLAGS': c['REINA_SNAP_FLAG_TESTING_EVER'] if testing_ever else 0,
          'LEN_Q0': qlen[0], 'LEN_Q1': qlen[1], 'LEN_L1': qlen[2]}
    for k, v in hd.items():
        words[c['REINA_SNAP_H_' + k]] = v
    ages = np.ascontiguousarray(np.array(config.age_start, dtype=np.int32)).tobytes()
    for k, v in (('AGES_HASH', _fnv1a64(ages)), ('DISEASE_HASH', _fnv1a64(bytes(disease))), ('BYTES', 4 * len(words))):
        words[c['REINA_SNAP_H_' + k]], words[c['REINA_SNAP_H_' + k] + 1] = v % (1 << 32), v >> 32
    return np.array(words, dtype=np.uint32)


_CTX = {}


def oracle_context(n):
    if n not in _CTX:
        _CTX[n] = snap_util.make_context(n, engine_factory=par_backend.par_engine_factory)
    return _CTX[n]


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('pattern', snap_util.PATTERNS)
@pytest.mark.parametrize('queues', [False, True])
def test_numpy_format_equals_the_plain_reference(n, pattern, queues):
    ctx = oracle_context(n)
    e = ctx.engine
    assert e.config.n_agents == n
    testing_ever = queues   # (both flags, both queue forms)
    st = snap_util.synthetic_state(n, e.config.max_queue, pattern, queues=queues)
    snap_util.write_state(e, st)
    img = snapmod.pack_numpy(e, ctx._disease, testing_ever).view(np.uint32)
    ref = reference_image(e.config, ctx._disease, st, testing_ever)
    assert len(img) == len(ref)
    bad = np.flatnonzero(img != ref)
    assert len(bad) == 0, 'words %s differ: %s != %s' % (bad[:8], img[bad[:8]], ref[bad[:8]])
    h = snapmod.parse_header(img)
    assert h['n_base'] == int((st['hot'] != 0).sum()) and h['testing_ever'] == testing_ever
    if pattern == 'empty':
        lay = snapmod.layout(n, 0, 0, st['qlen'])
        assert lay['rb'] == lay['rs'] == lay['q']
    # the numpy unpacker over garbage leaves the canonical state; its image packs back byte for byte
    snap_util.fill_garbage(e)
    snapmod.unpack_numpy(e, ctx._disease, img.view(np.uint8))
    snap_util.assert_state_equals(snap_util.read_state(e), snap_util.canonical(st, n), st['qlen'])
    assert np.array_equal(snapmod.pack_numpy(e, ctx._disease, testing_ever), img.view(np.uint8))


def test_synthetic_patterns_reach_the_edges():
    """the patterns really produce the shapes the format tests are about"""
    n = 4099
    T = snap_util.n_tiles(n)
    rec = {p: snap_util.synthetic_state(n, n + 64, p)['hot'] != 0 for p in snap_util.PATTERNS}
    assert not rec['empty'].any() and rec['full'].all()
    assert 0.2 < rec['random'].mean() < 0.4
    for i in [0, 63, 64, 511, 512, n - 1] + [t * 512 + d for t in range(1, T) for d in (-1, 0)]:
        assert rec['edges'][i], i
    assert rec['edges'].sum() == 4 + 2 * (T - 1)
    per_tile = np.add.reduceat(rec['alternating'], np.arange(0, n, 512))
    assert list(per_tile[:4]) == [512, 0, 512, 0] and per_tile[-1] == n - 512 * (T - 1)   # (T = 9: the ragged tile is full)
    st = snap_util.synthetic_state(n, n + 64, 'full')
    assert (st['infectees'] != 0xFFFFFFFF).all()
    st = snap_util.synthetic_state(n, n + 64, 'random')
    r = st['hot'] != 0
    used = (st['infectees'][r] != 0xFFFFFFFF).sum(axis=1)
    assert used.min() == 0 and used.max() == 8
    # rank order: the used slots of a recorded agent come first
    assert np.all(np.sort(st['infectees'][r] == 0xFFFFFFFF, axis=1) == (st['infectees'][r] == 0xFFFFFFFF))
    assert (st['infectees'][~r] != 0xFFFFFFFF).any() and (st['cold'][~r][:, 2:] != snap_util.COLD_DEFAULT[2:]).any()


def test_header_hashes_are_fnv1a_64():
    """the published FNV-1a 64 test vectors (offset basis 0xCBF29CE484222325): version 1 of the format had a mistyped basis"""
    for data, want in ((b'', 0xCBF29CE484222325), (b'a', 0xAF63DC4C8601EC8C), (b'foobar', 0x85944171F73967E8)):
        assert _fnv1a64(data) == want, data
        assert snapmod.fnv1a64(data) == want, data


def test_header_declares_the_snapshot_functions_the_binding_uses():
    declared = sorted(set(re.findall(r'\b(reina_[a-z_]+)\s*\(', _header_text('reina_snapshot.h'))))
    assert declared == sorted('reina_' + f for f in snapmod.SNAPSHOT_FUNCTIONS)


def test_header_constants_equal_the_python_mirror():
    c = header_constants()
    mirror = dict(REINA_SNAPSHOT_VERSION=snapmod.SNAPSHOT_VERSION, REINA_SNAP_MAGIC=snapmod.MAGIC, REINA_SNAP_TILE=snapmod.TILE,
                  REINA_SNAP_HEADER_WORDS=snapmod.HEADER_WORDS, REINA_SNAP_RECORD_WORDS=snapmod.RECORD_WORDS,
                  REINA_SNAP_FLAG_TESTING_EVER=snapmod.FLAG_TESTING_EVER)
    for k in ('MAGIC', 'VERSION', 'N_AGENTS', 'NR_AGES', 'NR_VARIANTS', 'N_TILES', 'N_BASE', 'N_SLOT', 'FLAGS', 'LEN_Q0',
              'LEN_Q1', 'LEN_L1', 'AGES_HASH', 'DISEASE_HASH', 'BYTES'):
        mirror['REINA_SNAP_H_' + k] = getattr(snapmod, 'H_' + k)
    assert sorted(c) == sorted(mirror), 'a constant of the header without a Python mirror, or the reverse'
    for k, v in mirror.items():
        assert c[k] == v, k
    assert c['REINA_SNAP_MAGIC'].to_bytes(4, 'little') == b'RSNP'
    # the header's word indices leave the two-word fields their two words
    words = sorted(v for k, v in c.items() if k.startswith('REINA_SNAP_H_'))
    assert words == list(range(12)) + [12, 14, 16]
    # the queue lengths of the control block, from reina_hip.h
    m = re.search(r'REINA_L_WORK\s*=\s*0\s*,\s*REINA_L_CAND\s*,\s*REINA_L_QUEUE0\s*,\s*REINA_L_QUEUE1\s*,\s*REINA_L_LEVEL1\b',
                  _header_text('reina_hip.h'))
    assert m and snapmod.L_QUEUE0 == 2


def test_library_exports_the_snapshot_functions():
    from reina_model_amd import build
    build.build()
    lib = eng.load_hip_library()
    for f in snapmod.SNAPSHOT_FUNCTIONS:
        assert hasattr(lib, 'reina_' + f), f
    f = snapmod.bind_snapshot_abi(lib, 'reina_')
    assert f is not None and f['snapshot_version']() == snapmod.SNAPSHOT_VERSION
