"""Device-side known-answer tests of the numeric primitives (reina_model_amd/csrc/reina_prims.h): the DEVICE build of
Philox4x32-10 / Philox2x32-10 / inverse normal / exp / log / gamma / the contact-count draw, evaluated one lane per record
through the C ABI's test hook (include/reina_hip.h: reina_test_prims), against

  * the published Random123 known-answer vectors (kat_vectors: philox4x32 10, philox2x32 10),
  * scipy / numpy in float64 (accuracy bounds -- the same bounds tests/test_prims.py holds the host build to),
  * the HOST build of the same header (oracle B's gcc compile) bit for bit on a million records each.

HIP == oracle B bit for bit (tests/test_parity_gpu.py) compares two programs that share this header; this file is what
pins the header's device compile itself (round-2 verdict, "What's weak")."""
import numpy as np
import pytest

import par_backend
from reina_model_amd import engine as eng
from test_prims import GAMMA_BUNDLED, GAMMA_GRID

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    return eng.bind_abi(eng.load_hip_library(), 'reina_')


@pytest.fixture(scope='module')
def host():
    return eng.bind_abi(par_backend.lib(), 'par_')


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def test_philox4x32_known_answers_on_the_device(dev, host):
    kat = [([0, 0, 0, 0, 0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
           ([0xffffffff] * 6, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
           ([0xa4093822, 0x299f31d0, 0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]
    out = eng.test_prims(dev, 'philox4', [k for k, _ in kat])
    for row, (_, want) in zip(out, kat):
        assert [int(x) for x in row] == want
    rec = np.random.default_rng(1).integers(0, 2 ** 32, size=(1 << 20, 6), dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(eng.test_prims(dev, 'philox4', rec), eng.test_prims(host, 'philox4', rec))


def test_philox2x32_known_answers_on_the_device(dev, host):
    kat = [([0, 0, 0], [0xff1dae59, 0x6cd10df2]), ([0xffffffff] * 3, [0x2c3f628b, 0xab4fd7ad]),
           ([0x13198a2e, 0x243f6a88, 0x85a308d3], [0xdd7ce038, 0xf62a4c12])]   # (key, ctr0, ctr1) -> (out0, out1)
    out = eng.test_prims(dev, 'philox2', [k for k, _ in kat])
    for row, (_, want) in zip(out, kat):
        assert [int(x) for x in row] == want
    rec = np.random.default_rng(2).integers(0, 2 ** 32, size=(1 << 20, 3), dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(eng.test_prims(dev, 'philox2', rec), eng.test_prims(host, 'philox2', rec))


def test_inverse_normal_on_the_device(dev, host):
    from scipy.special import ndtri
    r = np.concatenate([np.linspace(0, 2 ** 32 - 1, 1000001).astype(np.uint64),
                        np.arange(0, 4096, dtype=np.uint64), np.uint64(2 ** 32 - 1) - np.arange(0, 4096, dtype=np.uint64),
                        np.random.default_rng(3).integers(0, 2 ** 32, size=1 << 20, dtype=np.uint64)]).astype(np.uint32)
    d = eng.test_prims(dev, 'normal', r)[:, 0]
    assert np.array_equal(d, eng.test_prims(host, 'normal', r)[:, 0])   # every branch: both tails, the centre, the seam cells
    y = d.view(np.float32)
    ref = ndtri((r.astype(np.float64) + 0.5) / 2 ** 32)
    assert np.max(np.abs(y - ref)) < 2e-6


def test_expf_logf_on_the_device(dev, host):
    x = np.concatenate([np.linspace(-20, 20, 400001), np.linspace(-87, 88, 100001)]).astype(np.float32)
    d = eng.test_prims(dev, 'expf', _bits(x))[:, 0]
    assert np.array_equal(d, eng.test_prims(host, 'expf', _bits(x))[:, 0])
    ok = np.abs(x) <= 20
    ref = np.exp(x[ok].astype(np.float64))
    assert np.max(np.abs(d.view(np.float32)[ok] - ref) / ref) < 2e-7
    x = np.exp(np.linspace(-40, 40, 400001)).astype(np.float32)
    d = eng.test_prims(dev, 'logf', _bits(x))[:, 0]
    assert np.array_equal(d, eng.test_prims(host, 'logf', _bits(x))[:, 0])
    assert np.max(np.abs(d.view(np.float32) - np.log(x.astype(np.float64)))) < 4e-6


@pytest.mark.parametrize('mu,cv', GAMMA_BUNDLED + GAMMA_GRID)
def test_gamma_on_the_device(dev, host, mu, cv):
    """the bundled means, and the grid float32(base) * float32(theta) a per-member disease block hands the draw"""
    n = 400000
    rec = np.zeros((n, 8), dtype=np.uint32)
    rec[:, 0], rec[:, 1] = _bits([mu])[0], _bits([cv])[0]
    rec[:, 2], rec[:, 3] = 99, 0x1234567      # key
    rec[:, 4] = np.arange(n)                  # who
    rec[:, 5], rec[:, 6], rec[:, 7] = 3, 3, 1   # day, purpose (RP_P_INFECT), first block
    d = eng.test_prims(dev, 'gamma', rec)[:, 0]
    assert np.array_equal(d, eng.test_prims(host, 'gamma', rec)[:, 0])   # rejection loops and all
    g = d.view(np.float32)
    assert abs(g.mean() - mu) < 0.01 * mu and abs(g.std() / g.mean() - cv) < 0.01 and g.min() > 0 and np.all(np.isfinite(g))


def test_contact_count_draw_on_the_device(dev, host):
    """the 32-bit word the contact count is inverted from (rp_count_draw): Philox2x32 under its own key"""
    n = 1 << 19
    rng = np.random.default_rng(4)
    rec = np.zeros((n, 4), dtype=np.uint32)
    rec[:, 0], rec[:, 1] = 5, 77
    rec[:, 2] = np.arange(n)
    rec[:, 3] = rng.integers(0, 365, size=n)
    d = eng.test_prims(dev, 'count_draw', rec)[:, 0]
    assert np.array_equal(d, eng.test_prims(host, 'count_draw', rec)[:, 0])
    assert abs(d.astype(np.float64).mean() / 2 ** 32 - 0.5) < 0.002
