"""Snapshots of a running simulation, taken between two days (include/reina_snapshot.h; DESIGN.md "Snapshots").

A `Snapshot` holds
  * the engine image: one block of little-endian 32-bit words (header, counter and control blocks, per-512-agent-tile offset
    tables, one 32-byte record per agent whose hot word is non-zero, the inline infectee slots of those that have any, the
    test queues) -- on the device (a torch uint8 tensor, packed by the library's kernels) or on the host (a numpy uint8 array);
  * the Context's host state (day, seed, testing and vaccination settings, weekly-import bookkeeping, the contact matrix's
    mobility and mask state, a digest of the interventions applied so far) as a JSON-able dict;
  * optionally the counter history and mobility history of the days before it (simulation.simulate_with_snapshots).

This module also holds a numpy packer / unpacker of the same format: the format's executable specification, and the path
for engines whose state lives in host memory (engine.NumpyAllocator).  Files are written without pickle:
  b'RSNPFILE' | u64 length of the JSON text | JSON text | zero bytes to a multiple of 16 | image | history (int32).
"""
import ctypes
import json
import struct

import numpy as np

from . import engine as _eng
from . import reports as _rep

SNAPSHOT_VERSION = 2           # include/reina_snapshot.h: REINA_SNAPSHOT_VERSION
MAGIC = 0x504E5352             # "RSNP"
TILE = 512
HEADER_WORDS = 64
RECORD_WORDS = 8
(H_MAGIC, H_VERSION, H_N_AGENTS, H_NR_AGES, H_NR_VARIANTS, H_N_TILES, H_N_BASE, H_N_SLOT, H_FLAGS,
 H_LEN_Q0, H_LEN_Q1, H_LEN_L1) = range(12)
H_AGES_HASH, H_DISEASE_HASH, H_BYTES = 12, 14, 16
FLAG_TESTING_EVER = 1
L_QUEUE0 = 2                   # REINA_L_QUEUE0 (queue1, level1 follow)
FILE_MAGIC = b'RSNPFILE'
HOST_STATE_FORMAT = 1

SNAPSHOT_FUNCTIONS = ('snapshot_version', 'snap_measure', 'snap_pack', 'snap_unpack', 'group_snap_unpack')
_vp = ctypes.c_void_p
_SNAPSHOT_ARGTYPES = {'snap_measure': [_vp, ctypes.POINTER(ctypes.c_uint64), _vp], 'snap_pack': [_vp, _vp, ctypes.c_uint64, _vp],
                      'snap_unpack': [_vp, _vp, _vp], 'group_snap_unpack': [_vp, _vp, _vp]}


def bind_snapshot_abi(lib, prefix):
    """The snapshot entry points of a library, or None when it has none (a library of the day ABI only)."""
    return _eng.bind_optional_abi(lib, prefix, SNAPSHOT_FUNCTIONS, _SNAPSHOT_ARGTYPES, 'snapshot_version', SNAPSHOT_VERSION)


def fnv1a64(data):
    h = 14695981039346656037   # (FNV-1a 64: offset basis 0xCBF29CE484222325, prime 2^40 + 2^8 + 0xB3)
    for b in bytes(data):
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def layout(n_agents, n_base, n_slot, qlen):
    """word offsets of an image's sections (include/reina_snapshot.h)"""
    T = (int(n_agents) + TILE - 1) // TILE
    tb = HEADER_WORDS + _eng.COUNTER_WORDS + _eng.L_NR
    ts = tb + T + 1
    pad = ts + T + 1
    rb = (pad + 7) & ~7
    rs = rb + RECORD_WORDS * int(n_base)
    q = rs + RECORD_WORDS * int(n_slot)
    return dict(n_tiles=T, tb=tb, ts=ts, pad=pad, rb=rb, rs=rs, q=q, words=q + sum(int(x) for x in qlen))


def fixed_bytes(n_agents, qlen=(0, 0, 0)):
    """bytes of an image without any record: header, dense blocks, tile tables, queues"""
    return 4 * layout(n_agents, 0, 0, qlen)['words']


def expected_header(config, disease, n_base, n_slot, qlen, testing_ever):
    """the header words an image of an engine with this config and disease carries"""
    lay = layout(config.n_agents, n_base, n_slot, qlen)
    h = np.zeros(HEADER_WORDS, dtype=np.uint32)
    h[H_MAGIC], h[H_VERSION] = MAGIC, SNAPSHOT_VERSION
    h[H_N_AGENTS], h[H_NR_AGES], h[H_NR_VARIANTS] = config.n_agents, config.nr_ages, config.nr_variants
    h[H_N_TILES], h[H_N_BASE], h[H_N_SLOT] = lay['n_tiles'], n_base, n_slot
    h[H_FLAGS] = FLAG_TESTING_EVER if testing_ever else 0
    h[H_LEN_Q0:H_LEN_L1 + 1] = qlen
    for at, v in ((H_AGES_HASH, fnv1a64(bytes(config.age_start))), (H_DISEASE_HASH, fnv1a64(bytes(disease))),
                  (H_BYTES, 4 * lay['words'])):
        h[at], h[at + 1] = v & 0xFFFFFFFF, v >> 32
    return h


def parse_header(words):
    w = [int(x) for x in np.asarray(words, dtype=np.uint32)[:HEADER_WORDS]]
    return dict(magic=w[H_MAGIC], version=w[H_VERSION], n_agents=w[H_N_AGENTS], nr_ages=w[H_NR_AGES],
                nr_variants=w[H_NR_VARIANTS], n_tiles=w[H_N_TILES], n_base=w[H_N_BASE], n_slot=w[H_N_SLOT],
                testing_ever=bool(w[H_FLAGS] & FLAG_TESTING_EVER), qlen=(w[H_LEN_Q0], w[H_LEN_Q1], w[H_LEN_L1]),
                ages_hash=w[H_AGES_HASH] | w[H_AGES_HASH + 1] << 32, disease_hash=w[H_DISEASE_HASH] | w[H_DISEASE_HASH + 1] << 32,
                bytes=w[H_BYTES] | w[H_BYTES + 1] << 32)


def check_compatible(config, disease, header):
    """ValueError unless an image with `header` can be restored into an engine of (config, disease)"""
    if config.n_shards > 1:
        raise ValueError('snapshots are restored into unsharded Contexts only')
    if header['magic'] != MAGIC or header['version'] != SNAPSHOT_VERSION:
        raise ValueError('not a snapshot image of format version %d' % SNAPSHOT_VERSION)
    if header['n_agents'] != config.n_agents or header['nr_ages'] != config.nr_ages \
            or header['ages_hash'] != fnv1a64(bytes(config.age_start)):
        raise ValueError('snapshot of another population')
    if header['nr_variants'] != config.nr_variants:
        raise ValueError('snapshot with another number of variants')
    if header['disease_hash'] != fnv1a64(bytes(disease)):
        raise ValueError('snapshot of another disease')
    if header['n_base'] > config.n_agents or header['n_slot'] > header['n_base'] or max(header['qlen']) > config.max_queue:
        raise ValueError('snapshot counts out of range')
    if header['bytes'] != 4 * layout(config.n_agents, header['n_base'], header['n_slot'], header['qlen'])['words']:
        raise ValueError('snapshot image size does not match its header')


def _host_views(engine):
    t = engine.tensors
    n = engine.config.n_agents
    return (np.asarray(t['hot']).view(np.uint32), np.asarray(t['cold']).view(np.uint32).reshape(n, _eng.COLD_WORDS),
            np.asarray(t['infectees']).view(np.uint32).reshape(n, _eng.INLINE_INFECTEES))


def pack_numpy(engine, disease, testing_ever):
    """The image of a host-memory engine (numpy arrays), word for word what reina_snap_pack writes."""
    t = engine.tensors
    hot, cold, inf = _host_views(engine)
    n = engine.config.n_agents
    control = np.asarray(t['control']).view(np.uint32)
    qlen = [int(np.asarray(t['control'])[L_QUEUE0 + k]) for k in range(3)]
    if min(qlen) < 0 or max(qlen) > engine.config.max_queue:
        raise ValueError('a queue length of the control block is out of range')
    rec = np.flatnonzero(hot).astype(np.uint32)
    has = inf[rec, 0] != 0xFFFFFFFF        # (the inline slots are filled in rank order)
    lay = layout(n, len(rec), int(has.sum()), qlen)
    T = lay['n_tiles']
    img = np.zeros(lay['words'], dtype=np.uint32)
    img[:HEADER_WORDS] = expected_header(engine.config, disease, len(rec), int(has.sum()), qlen, testing_ever)
    img[HEADER_WORDS:HEADER_WORDS + _eng.COUNTER_WORDS] = np.asarray(t['counters']).view(np.uint32)
    img[HEADER_WORDS + _eng.COUNTER_WORDS:lay['tb']] = control
    tiles = rec >> 9
    for at, sel in ((lay['tb'], tiles), (lay['ts'], tiles[has])):
        img[at + 1:at + T + 1] = np.cumsum(np.bincount(sel, minlength=T))
    base = img[lay['rb']:lay['rs']].reshape(-1, RECORD_WORDS)
    base[:, 0] = rec | (has.astype(np.uint32) << 31)
    base[:, 1] = hot[rec]
    base[:, 2:] = cold[rec, 2:]
    img[lay['rs']:lay['q']].reshape(-1, RECORD_WORDS)[:] = inf[rec[has]]
    q = lay['q']
    for k, name in enumerate(('queue0', 'queue1', 'level1')):
        img[q:q + qlen[k]] = np.asarray(t[name]).view(np.uint32)[:qlen[k]]
        q += qlen[k]
    return img.view(np.uint8)


def unpack_numpy(engine, disease, image):
    """Restore an image into a host-memory engine: k_init's defaults, the records over them, the dense blocks, both bit
    planes (what k_snap_unpack does).  Returns the header."""
    words = np.ascontiguousarray(image).view(np.uint32)
    h = parse_header(words)
    check_compatible(engine.config, disease, h)
    if len(words) * 4 < h['bytes']:
        raise ValueError('snapshot image shorter than its header says')
    t = engine.tensors
    hot, cold, inf = _host_views(engine)
    n = engine.config.n_agents
    lay = layout(n, h['n_base'], h['n_slot'], h['qlen'])
    base = words[lay['rb']:lay['rs']].reshape(-1, RECORD_WORDS)
    slots = words[lay['rs']:lay['q']].reshape(-1, RECORD_WORDS)
    idx = (base[:, 0] & 0x7FFFFFFF).astype(np.int64)
    has = (base[:, 0] >> 31) != 0
    if len(idx) and (idx.max() >= n or np.any(np.diff(idx) <= 0)) or int(has.sum()) != len(slots):
        raise ValueError('snapshot records out of order or out of range')
    hot[:] = 0
    cold[:] = np.array([0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF], dtype=np.uint32)
    inf[:] = 0xFFFFFFFF
    hot[idx] = base[:, 1]
    cold[idx, 2:] = base[:, 2:]
    inf[idx[has]] = slots
    np.asarray(t['counters']).view(np.uint32)[:] = words[HEADER_WORDS:HEADER_WORDS + _eng.COUNTER_WORDS]
    np.asarray(t['control']).view(np.uint32)[:] = words[HEADER_WORDS + _eng.COUNTER_WORDS:lay['tb']]
    q = lay['q']
    for k, name in enumerate(('queue0', 'queue1', 'level1')):
        np.asarray(t[name]).view(np.uint32)[:h['qlen'][k]] = words[q:q + h['qlen'][k]]
        q += h['qlen'][k]
    for name, bit in (('active_bits', (hot & 0x8000) != 0), ('infected_bits', (hot & 7) != 0)):
        plane = np.asarray(t[name]).view(np.uint32)
        plane[:] = 0
        packed = np.packbits(bit, bitorder='little')
        plane.view(np.uint8)[:len(packed)] = packed
    return h


def _snap_f(engine):
    return _rep.entry_points(engine, 'snap_f', 'snapshot', 'reina_snapshot.h')


def pack_engine(engine, disease, testing_ever):
    """The engine's image: packed by the library's kernels into a device tensor (HIP engine), by pack_numpy otherwise."""
    if not _eng.is_device(engine):
        return pack_numpy(engine, disease, testing_ever)
    f = _snap_f(engine)
    torch = engine.alloc.torch
    nbytes = ctypes.c_uint64()
    stream = engine.alloc.stream()
    engine._check(f['snap_measure'](engine._h, ctypes.byref(nbytes), stream), 'snap_measure')
    out = torch.empty(int(nbytes.value), dtype=torch.uint8, device=engine.alloc.device)
    engine._check(f['snap_pack'](engine._h, out.data_ptr(), int(nbytes.value), stream), 'snap_pack')
    return out


def _device_image(alloc, image):
    torch = alloc.torch
    if isinstance(image, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(image.view(np.uint8))).to(alloc.device)
    return image if image.device == alloc.device else image.to(alloc.device)


def _host_image(image):
    if isinstance(image, np.ndarray):
        return image
    return image.cpu().numpy()


def _check_image_length(dev):
    """the library reads as many bytes as the image's header says: the buffer must hold them"""
    if str(dev.dtype) != 'torch.uint8' or not dev.is_contiguous():
        raise ValueError('a snapshot image is a contiguous uint8 tensor')
    if dev.numel() < 4 * HEADER_WORDS or dev.numel() < parse_header(dev[:4 * HEADER_WORDS].cpu().numpy().view(np.uint32))['bytes']:
        raise ValueError('snapshot image shorter than its header says')


def unpack_engine(engine, disease, image):
    """Restore `image` (host or device) into one engine."""
    if not _eng.is_device(engine):
        return unpack_numpy(engine, disease, _host_image(image))
    f = _snap_f(engine)
    dev = _device_image(engine.alloc, image)
    _check_image_length(dev)
    engine._check(f['snap_unpack'](engine._h, dev.data_ptr(), engine.alloc.stream()), 'snap_unpack')
    engine._keep_image = dev   # (alive until the queued launch has read it; replaced by the next restore)
    return None


def unpack_group(group, disease, image):
    """Restore `image` into every member of an engine group: ONE launch on the device (reina_group_snap_unpack), the numpy
    unpacker per member for host-memory engines."""
    e0 = group.engines[0]
    if not _eng.is_device(e0):
        for e in group.engines:
            unpack_numpy(e, disease, _host_image(image))
        return
    f = _snap_f(e0)
    dev = _device_image(e0.alloc, image)
    _check_image_length(dev)
    e0._check(f['group_snap_unpack'](group._h, dev.data_ptr(), e0.alloc.stream()), 'group_snap_unpack')
    _eng.mark_stale(group.engines)
    for e in group.engines:
        e._keep_image = dev


class Snapshot:
    """A simulation between two days: engine image + the Context's host state (+ optionally the history before it)."""

    def __init__(self, image, state, history=None, mobility_history=None):
        self.image = image
        self.state = state
        self.history = history
        self.mobility_history = mobility_history
        words = _host_image(image[:4 * HEADER_WORDS]) if not isinstance(image, np.ndarray) else image[:4 * HEADER_WORDS]
        self.header = parse_header(np.ascontiguousarray(words).view(np.uint32))

    @property
    def day(self):
        return int(self.state['day'])

    @property
    def seed(self):
        return int(self.state['seed'])

    @property
    def nbytes(self):
        return int(self.header['bytes'])

    @property
    def on_device(self):
        return not isinstance(self.image, np.ndarray)

    def to_host(self):
        """the same snapshot with its image in host memory"""
        return Snapshot(np.array(_host_image(self.image), copy=True), self.state, self.history, self.mobility_history)

    def with_history(self, history, mobility_history):
        return Snapshot(self.image, self.state, history, mobility_history)

    def save(self, path):
        img = np.ascontiguousarray(_host_image(self.image)).view(np.uint8)
        hist = None if self.history is None else np.ascontiguousarray(self.history, dtype=np.int32)
        meta = dict(state=self.state, image_bytes=int(img.nbytes),
                    history_rows=None if hist is None else int(hist.shape[0]),
                    mobility_history=None if self.mobility_history is None else [float(x) for x in self.mobility_history])
        text = json.dumps(meta).encode()
        head = FILE_MAGIC + struct.pack('<Q', len(text)) + text
        with open(path, 'wb') as fh:
            fh.write(head + b'\0' * (-len(head) % 16))
            fh.write(img.tobytes())
            if hist is not None:
                fh.write(hist.tobytes())

    @classmethod
    def load(cls, path, device=None):
        """`device`: None keeps the image in host memory, else a torch device to put it on"""
        with open(path, 'rb') as fh:
            data = fh.read()
        if data[:8] != FILE_MAGIC:
            raise ValueError('%s: not a snapshot file' % path)
        (n,) = struct.unpack('<Q', data[8:16])
        meta = json.loads(data[16:16 + n].decode())
        at = 16 + n
        at += -at % 16
        img = np.frombuffer(data, dtype=np.uint8, count=meta['image_bytes'], offset=at).copy()
        at += meta['image_bytes']
        hist = None
        if meta['history_rows'] is not None:
            hist = np.frombuffer(data, dtype=np.int32, count=meta['history_rows'] * _eng.COUNTER_WORDS, offset=at)
            hist = hist.reshape(meta['history_rows'], _eng.COUNTER_WORDS).copy()
        image = img
        if device is not None:
            import torch
            image = torch.from_numpy(img).to(device)
        return cls(image, meta['state'], hist, meta['mobility_history'])
