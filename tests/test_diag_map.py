"""The slot map of the diagnostic builds (reina_model_amd/csrc/reina_diag.h) on the CPU: the map part of the header compiled alone
by the host compiler, with EVERY switch defined at once, behind a small extern "C" shim (the pattern of tests/test_launch_plan.py).

The diagnostic builds are no part of the suite -- a variant takes a minute to compile and none is built here -- so what the
header's static_asserts say is said again from outside, on the tables themselves: regions share no word whatever the switches, end
inside buffers.mirror as engine.py allocates it, phases have one name each; and the text a diagnostic library hands to
tools/diag.py (reina_diag_describe) parses back, with the tool's own parser, to exactly the map."""
import ctypes
import os
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)
from reina_model_amd import engine as eng  # noqa: E402
import diag  # noqa: E402

HEADER = os.path.join(ROOT, 'reina_model_amd', 'csrc', 'reina_diag.h')
PROF_PART = 9
SWITCHES = ['REINA_' + s for s in diag.STAMPS] + ['REINA_ABLATE', 'REINA_DAY_PROF=%d' % PROF_PART]
KINDS = {1: 'SUM', 2: 'MAX', 4: 'COUNT', 8: 'ROWS'}
SHIM = r'''
#include "%s"
extern "C" {
size_t reina_diag_describe(char *out, size_t cap) { return diag_describe(out, cap); }
int shim_constant(int k) {
    const int c[] = {DIAG_N_REGIONS, DIAG_N_PHASES, DIAG_MIRROR_WORDS, DIAG_ROW_WORDS, (int)(sizeof(DIAG_PROF_TABLE) / sizeof(DiagName)),
                     (int)(sizeof(DIAG_ABLATE_TABLE) / sizeof(DiagName)), DIAG_PROF_PART};
    return c[k];
}
const DiagRegion *shim_region(int r) { return &DIAG_REGION_TABLE[r]; }
const DiagPhase *shim_phase(int q) { return &DIAG_PHASE_TABLE[q]; }
int shim_phase_word(int q) { return diag_phase_word(q); }
const DiagName *shim_part(int k) { return &DIAG_PROF_TABLE[k]; }
const DiagName *shim_bit(int k) { return &DIAG_ABLATE_TABLE[k]; }
}
'''


class Region(ctypes.Structure):
    _fields_ = [('name', ctypes.c_char_p), ('sw', ctypes.c_char_p), ('first', ctypes.c_int), ('words', ctypes.c_int), ('on', ctypes.c_int)]


class Phase(ctypes.Structure):
    _fields_ = [('region', ctypes.c_int), ('name', ctypes.c_char_p), ('kinds', ctypes.c_int)]


class Name(ctypes.Structure):
    _fields_ = [('name', ctypes.c_char_p), ('value', ctypes.c_int)]


@pytest.fixture(scope='module')
def shim():
    tmp = tempfile.mkdtemp(prefix='reina_diag_')
    src, so = os.path.join(tmp, 'shim.cpp'), os.path.join(tmp, 'libshim.so')
    with open(src, 'w') as f:
        f.write(SHIM % HEADER)
    subprocess.run(['g++', '-O1', '-std=c++17', '-Wall', '-Werror', '-Wno-unused-function', '-fPIC', '-shared'] + ['-D' + s for s in SWITCHES] +
                   ['-o', so, src], check=True)
    lib = ctypes.CDLL(so)
    lib.shim_region.restype = ctypes.POINTER(Region)
    lib.shim_phase.restype = ctypes.POINTER(Phase)
    lib.shim_part.restype = lib.shim_bit.restype = ctypes.POINTER(Name)
    return lib


@pytest.fixture(scope='module')
def tables(shim):
    """the header's tables as they stand: regions [(name, switch, first, words, on)], phases [(region name, phase, kinds, first word)]"""
    regions = [shim.shim_region(r).contents for r in range(shim.shim_constant(0))]
    regions = [(r.name.decode(), r.sw.decode(), r.first, r.words, r.on) for r in regions]
    phases = [(shim.shim_phase(q).contents, shim.shim_phase_word(q)) for q in range(shim.shim_constant(1))]
    phases = [(regions[p.region][0], p.name.decode(), p.kinds, w) for p, w in phases]
    return regions, phases


def test_regions_are_disjoint_and_inside_the_buffer(shim, tables):
    regions, _ = tables
    assert shim.shim_constant(2) == eng.DIAG_MIRROR_WORDS
    assert len({r[0] for r in regions}) == len(regions)
    for k, (name, _, first, words, on) in enumerate(regions):
        assert first >= 0 and words > 0 and first + words <= eng.DIAG_MIRROR_WORDS, name
        assert on == 1, name   # (every switch is defined: every region is written)
        for other, _, f2, w2, _ in regions[k + 1:]:
            assert first + words <= f2 or f2 + w2 <= first, (name, other)


def test_phases_have_one_name_each_and_fill_their_region(shim, tables):
    regions, phases = tables
    row = shim.shim_constant(3)
    for name, _, first, words, _ in regions:
        mine = [p for p in phases if p[0] == name]
        assert mine and len({p[1] for p in mine}) == len(mine), name
        taken = []
        for _, ph, kinds, word in mine:
            assert kinds and not kinds & ~15 and (kinds == 8 or not kinds & 8), (name, ph)
            taken += range(word, word + bin(kinds).count('1'))
        if mine[0][2] == 8:   # whole rows, one word of the row per phase
            assert all(p[2] == 8 for p in mine) and taken == list(range(first, first + row)) and words % row == 0, name
        else:
            assert taken == list(range(first, first + words)), name


def test_the_text_parses_back_to_the_map(shim, tables):
    regions, phases = tables
    m = diag.describe(shim)
    assert m['regions'] == {name: (sw, first, words, on) for name, sw, first, words, on in regions}
    words = []
    for name, ph, kinds, word in phases:
        for bit in (1, 2, 4, 8):
            if kinds & bit:
                words.append((word, name, ph, KINDS[bit]))
                word += 1
    assert m['words'] == words
    assert len({w for w, r, _, _ in m['words']}) == len(m['words'])
    assert m['row'] == shim.shim_constant(3)
    assert sorted(m['switches']) == sorted(s.split('=')[0] for s in SWITCHES) and m['prof'] == PROF_PART == shim.shim_constant(6)
    parts = {shim.shim_part(k).contents.name.decode(): shim.shim_part(k).contents.value for k in range(shim.shim_constant(4))}
    bits = {shim.shim_bit(k).contents.name.decode(): shim.shim_bit(k).contents.value for k in range(shim.shim_constant(5))}
    assert m['part'] == parts and sorted(parts.values()) == list(range(18))
    assert m['bit'] == bits and sorted(bits.values()) == [1 << k for k in range(8)]
    assert diag.number_of(m['bit'], 'RESOLVE+CONTACTS') == 5 and diag.number_of(m['bit'], '56') == 56


def test_a_short_buffer_is_cut_and_terminated(shim):
    shim.reina_diag_describe.restype = ctypes.c_size_t
    shim.reina_diag_describe.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    whole = shim.reina_diag_describe(None, 0)
    buf = ctypes.create_string_buffer(b'\xff' * 64, 64)
    assert shim.reina_diag_describe(buf, 40) == whole > 40
    assert len(buf.value) == 39 and buf.raw[40:] == b'\xff' * 24
