"""The snapshot kernels (k_snap_count / k_snap_scan / k_snap_pack / k_snap_unpack<GROUP>) against the numpy packer and
unpacker (snapshot.pack_numpy / unpack_numpy, the format's executable specification) on synthetic states
(tests/snap_util.py) at the shapes where they could break: populations of one agent, of less than a wave, of whole and
ragged tiles, and of 1023 / 1024 / 1025 / 3293 tiles (the one-workgroup scan's chunking); empty, full, random, tile-edge
and alternating records; unpacking over garbage; the group unpack's member chunks along blockIdx.y.

A synthetic state's hot words and indices are garbage: it only goes through pack and unpack, never through a day."""
import ctypes

import numpy as np
import pytest

import par_backend
import snap_util
from reina_model_amd import engine as eng
from reina_model_amd import snapshot as snapmod

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 511, 512, 513, 4099, 29_993, 523_776, 524_288, 524_289, 1_685_983)
# (queues, testing_ever) per pattern: each of the four forms of the image's tail and flag at every size
FORMS = dict(empty=(True, True), full=(False, False), random=(True, True), edges=(False, True), alternating=(True, False))

_CTX = {}


def _contexts(n):
    """(oracle-B Context, HIP Context) of n agents; one size kept at a time"""
    if n not in _CTX:
        _CTX.clear()
        _CTX[n] = (snap_util.make_context(n, engine_factory=par_backend.par_engine_factory), snap_util.make_context(n))
    return _CTX[n]


def _state_and_image(cpu, pattern):
    e = cpu.engine
    queues, testing_ever = FORMS[pattern]
    st = snap_util.synthetic_state(e.config.n_agents, e.config.max_queue, pattern, queues=queues)
    snap_util.write_state(e, st)
    return st, snapmod.pack_numpy(e, cpu._disease, testing_ever)


def _gpu_image(gpu):
    return snapmod.pack_engine(gpu.engine, gpu._disease, None).cpu().numpy()


def _measure(engine):
    nbytes = ctypes.c_uint64()
    engine._check(engine.snap_f['snap_measure'](engine._h, ctypes.byref(nbytes), engine.alloc.stream()), 'snap_measure')
    return int(nbytes.value)


def _assert_same_bytes(got, want, what):
    assert len(got) == len(want), '%s: %d bytes, the format has %d' % (what, len(got), len(want))
    g, w = got.view(np.uint32), want.view(np.uint32)
    bad = np.flatnonzero(g != w)
    assert len(bad) == 0, '%s: %d words differ, first at %s: %s != %s' % (what, len(bad), bad[:4], g[bad[:4]], w[bad[:4]])


def test_sizes_reach_the_scan_shapes():
    T = {n: snap_util.n_tiles(n) for n in SIZES}
    assert T[523_776] == 1023 and T[524_288] == 1024 and T[524_289] == 1025 and T[1_685_983] == 3293
    per = lambda t: -(-t // 1024)
    assert per(1025) == 2 and 1024 - -(-1025 // 2) == 511 and per(3293) == 4   # (1025 tiles: 511 threads of the scan empty)


@pytest.mark.parametrize('pattern', snap_util.PATTERNS)
@pytest.mark.parametrize('n', SIZES)
def test_pack_equals_the_format(n, pattern):
    """the whole image -- header, counters, control, both tile tables, the pad, both record streams, the queues -- is
    pack_numpy's, byte for byte; snap_measure says its size; a second pack writes the same bytes"""
    cpu, gpu = _contexts(n)
    st, want = _state_and_image(cpu, pattern)
    # the engine's testing_ever flag is host state that only a day or a restore sets: restore the image, then put the raw
    # synthetic state (garbage claims and slots of unrecorded agents, queue words past their lengths) over it
    snapmod.unpack_engine(gpu.engine, gpu._disease, want)
    snap_util.write_state(gpu.engine, st)
    assert _measure(gpu.engine) == len(want)
    got = _gpu_image(gpu)
    _assert_same_bytes(got, want, 'pack')
    _assert_same_bytes(_gpu_image(gpu), got, 'second pack')
    h = snapmod.parse_header(got.view(np.uint32))
    assert h['n_base'] == int((st['hot'] != 0).sum()) and h['testing_ever'] == FORMS[pattern][1]


@pytest.mark.parametrize('pattern', snap_util.PATTERNS)
@pytest.mark.parametrize('n', SIZES)
def test_unpack_equals_the_format(n, pattern):
    """unpacked over garbage, the engine holds unpack_numpy's state word for word: the per-agent arrays, the dense blocks,
    the queues up to their lengths, both bit planes (the padding tile still 0); and packs back to the same bytes"""
    cpu, gpu = _contexts(n)
    st, img = _state_and_image(cpu, pattern)
    snap_util.fill_garbage(cpu.engine)
    snapmod.unpack_numpy(cpu.engine, cpu._disease, img)
    want = snap_util.read_state(cpu.engine)
    snap_util.assert_state_equals(want, snap_util.canonical(st, n), st['qlen'])
    snap_util.fill_garbage(gpu.engine)
    snapmod.unpack_engine(gpu.engine, gpu._disease, img)
    gpu.engine.alloc.torch.cuda.synchronize()
    snap_util.assert_state_equals(snap_util.read_state(gpu.engine), want, st['qlen'])
    _assert_same_bytes(_gpu_image(gpu), img, 'pack after unpack')


# (n, members, pattern, geometry the case is there for)
GROUP_CASES = [(1, 3, 'full', 'a member per chunk'), (29_993, 40, 'random', 'ragged'), (153_600, 10, 'alternating', 'ragged'),
               (29_993, 128, 'edges', 'many chunks'), (1_685_983, 5, 'random', 'one chunk')]


@pytest.mark.parametrize('n,members,pattern,geometry', GROUP_CASES)
def test_group_unpack_equals_the_format(n, members, pattern, geometry):
    """reina_group_snap_unpack over K garbage-filled engines: every member holds unpack_numpy's state and packs back to the
    image, whichever chunk of blockIdx.y wrote it"""
    import torch
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    chunks, per, last = snap_util.group_geometry(snap_util.n_tiles(n), members, n_cus)
    reached = {'a member per chunk': chunks == members and per == 1, 'ragged': chunks > 1 and last < per,
               'many chunks': chunks >= 8, 'one chunk': chunks == 1}[geometry]
    assert reached, (geometry, n_cus, chunks, per, last)
    cpu, gpu = _contexts(n)
    st, img = _state_and_image(cpu, pattern)
    snap_util.fill_garbage(cpu.engine)
    snapmod.unpack_numpy(cpu.engine, cpu._disease, img)
    want = snap_util.read_state(cpu.engine)
    engines = [eng.hip_engine(gpu.engine.config, gpu._disease) for _ in range(members)]
    group = eng.EngineGroup(engines)
    try:
        for e in engines:
            snap_util.fill_garbage(e)
        snapmod.unpack_group(group, gpu._disease, img)
        torch.cuda.synchronize()
        for m, e in enumerate(engines):
            try:
                snap_util.assert_state_equals(snap_util.read_state(e), want, st['qlen'])
            except AssertionError as x:
                raise AssertionError('member %d (chunk %d of %d): %s' % (m, m // per, chunks, x))
            _assert_same_bytes(snapmod.pack_engine(e, gpu._disease, None).cpu().numpy(), img, 'member %d packed back' % m)
    finally:
        group.close()
        for e in engines:
            e.close()
