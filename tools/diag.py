"""The diagnostic builds of the day kernels (reina_model_amd/csrc/reina_diag.h): build them, run them, read them back.

  python tools/diag.py build <switch ...>       one variant: OPEN_STAMPS, HOSP_STAMPS INSTALL_STAMPS, DAY_PROF=9 ABLATE, NO_BYBIT, ...
  python tools/diag.py build --all              every variant of VARIANTS below, at most 16 compiles at a time
  python tools/diag.py run <what> [agents] [lo:hi ...]

`run` loads the variant into this process (REINA_HIP_LIB, set before the package is imported), runs the default scenario -- the
HUS population, above 2 x 10^6 agents the scaled one of bench.py -- window by window with buffers.mirror zeroed in front of each,
and prints one line per window, then the SHA-256 of the hot words and of the counter block.  What a word of buffers.mirror means
comes from the library itself (reina_diag_describe): no offset is written here.  <what> and its default size and windows:
  open     OPEN_STAMPS: the opening's roles, the slowest tracing wave, the import placement (1e8; 0:118 118:200 200:365)
  imports  the same build on the import days (1e8; 0:20 20:21 21:196 196:197)
  hosp     HOSP_STAMPS + INSTALL_STAMPS: the small ordered event walk and the install roles (1e8; six windows around the peak)
  install  the same build (1e8; five windows); --group K: member 0 of an engine group of K HUS members (0:60 60:125 125:365)
  day      DAY_STAMPS: k_day's workgroups (HUS; six windows)
  small    SMALL_STAMPS: k_small_days with REINA_FUSED_DAY=1 (HUS; six windows); --wgs N sets REINA_FUSED_WGS
  prof P   DAY_PROF=P, a part's number (reina_diag.h: DIAG_PROF_PARTS; the line names it): cycles per wave of k_day on single days
           (1e8; 20:21 60:61 93:94 200:201) beside k_day's time
  ablate   ABLATE [--prof P]: runs to --start (ABLATE_START, 92), then --days days (3) per entry of --bits (names or numbers, summed
           with +: "0 RESOLVE CONTACTS+COUNT_DRAW"), kernel times from the HIP-event profile; with --prof the waves' rows as well
--raw adds every word as REGION.PHASE.KIND=<integer>."""
import argparse
import concurrent.futures
import copy
import ctypes
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VARIANT_DIR = os.path.join(ROOT, 'reina_model_amd', 'csrc', 'variants')
STAMPS = ('OPEN_STAMPS', 'HOSP_STAMPS', 'INSTALL_STAMPS', 'DAY_STAMPS', 'SMALL_STAMPS')
VARIANTS = [('DAY_PROF=1',), ('DAY_PROF=6',), ('DAY_PROF=9',), ('DAY_PROF=12', 'ABLATE'), ('DAY_PROF=17',), ('DAY_STAMPS',), ('OPEN_STAMPS',),
            ('HOSP_STAMPS', 'INSTALL_STAMPS'), ('SMALL_STAMPS',), ('ABLATE',), ('NO_BYBIT',), ('NO_DAY_PRIO',), STAMPS]
HUS_WINDOWS = '0:5 5:25 25:90 90:110 110:300 300:365'
RUNS = {   # what: (switches, default agents, default windows)
    'open': (('OPEN_STAMPS',), 1e8, '0:118 118:200 200:365'),
    'imports': (('OPEN_STAMPS',), 1e8, '0:20 20:21 21:196 196:197'),
    'hosp': (('HOSP_STAMPS', 'INSTALL_STAMPS'), 1e8, '0:60 60:85 85:100 100:125 125:160 160:365'),
    'install': (('HOSP_STAMPS', 'INSTALL_STAMPS'), 1e8, '0:60 60:85 85:125 125:160 160:365'),
    'day': (('DAY_STAMPS',), 1685983, HUS_WINDOWS),
    'small': (('SMALL_STAMPS',), 1685983, HUS_WINDOWS),
    'prof': (None, 1e8, '20:21 60:61 93:94 200:201'),
    'ablate': (None, 1e8, ''),
}


def switches_of(names):
    return sorted('REINA_' + n.upper().replace('REINA_', '', 1) for n in names)


def variant_path(names):
    return os.path.join(VARIANT_DIR, 'libreina_%s.so' % '+'.join(s[len('REINA_'):].lower() for s in switches_of(names)))


def build(names):
    from reina_model_amd.build import build_variant
    os.makedirs(VARIANT_DIR, exist_ok=True)
    return build_variant(switches_of(names), variant_path(names))


def describe(lib):
    """the library's own account of buffers.mirror: regions {name: (switch, first, words, on)}, words [(word, region, phase, kind)],
    part and bit numbers by name, the part this library times"""
    lib.reina_diag_describe.restype = ctypes.c_size_t
    lib.reina_diag_describe.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    buf = ctypes.create_string_buffer(lib.reina_diag_describe(None, 0) + 1)
    lib.reina_diag_describe(buf, len(buf))
    m = {'regions': {}, 'words': [], 'part': {}, 'bit': {}, 'switches': [], 'prof': -1}
    for f in (line.split() for line in buf.value.decode().splitlines()):
        if f[0] == 'region':
            m['regions'][f[1]] = (f[2], int(f[3]), int(f[4]), int(f[5]))
        elif f[0] == 'word':
            m['words'].append((int(f[1]), f[2], f[3], f[4]))
        elif f[0] in ('part', 'bit'):
            m[f[0]][f[2]] = int(f[1])
        elif f[0] == 'switches':
            m['switches'] = f[1:]
        elif f[0] == 'prof':
            m['prof'] = int(f[1])
        elif f[0] == 'mirror':
            m['row'] = int(f[3])
    return m


def number_of(table, text):
    """'RESOLVE+CONTACTS' or a plain number -> the number"""
    return sum(int(t) if t.isdigit() else table[t.upper()] for t in text.split('+'))


def window_line(m, mir, days, raw):
    """one window's words of every region this library writes, times in us (a tick is 10 ns; a ROWS region counts shader cycles)"""
    out = []
    for region, (_, first, words, on) in m['regions'].items():
        if not on:
            continue
        mine = [(w, ph, kind) for w, r, ph, kind in m['words'] if r == region]
        if mine[0][2] == 'ROWS':
            rows = mir[first:first + words].reshape(-1, m['row']).astype(float)
            col = {ph: rows[:, w - first] for w, ph, _ in mine}
            rows_n = int((col['WRITTEN'] > 0).sum())
            n = max(1, rows_n)
            out.append('%s: rows %d, per wave: loop %.1f kcycles (slowest %.1f), part %.1f kcycles in %.1f pieces' % (
                region, rows_n, col['LOOP'].sum() / n / 1e3, col['LOOP'].max() / 1e3, col['PART'].sum() / n / 1e3, col['PIECES'].sum() / n))
            continue
        val = {(ph, kind): int(mir[w]) for w, ph, kind in mine}
        parts = []
        for ph in dict.fromkeys(ph for _, ph, _ in mine):
            t = []
            if (ph, 'SUM') in val:
                t.append('%.2f/day' % (val[ph, 'SUM'] / 100.0 / days))
                if val.get((ph, 'COUNT')):
                    t.append('mean %.2f' % (val[ph, 'SUM'] / 100.0 / val[ph, 'COUNT']))
            if (ph, 'MAX') in val:
                t.append('max %.2f' % (val[ph, 'MAX'] / 100.0))
            if (ph, 'COUNT') in val:
                t.append('n=%d' % val[ph, 'COUNT'])
            parts.append('%s %s' % (ph, ' '.join(t)))
        out.append('%s: %s' % (region, ', '.join(parts)))
        if raw:
            out.append('raw ' + ' '.join('%s.%s.%s=%d' % (region, ph, kind, val[ph, kind]) for _, ph, kind in mine))
    return ' | '.join(out)


def run(a):
    names, agents, windows = RUNS[a.what]
    if a.what == 'prof':
        names = ('DAY_PROF=%s' % a.part,)
    if a.what == 'ablate':
        names = ('ABLATE',) + (('DAY_PROF=%s' % a.prof,) if a.prof else ())
    path = a.lib or variant_path(names)
    if not os.path.exists(path):
        sys.exit('%s is not built: python tools/diag.py build %s' % (path, ' '.join(names)))
    os.environ['REINA_HIP_LIB'] = path
    if a.what == 'small':
        os.environ.setdefault('REINA_FUSED_DAY', '1')
        if a.wgs:
            os.environ['REINA_FUSED_WGS'] = str(a.wgs)
    import numpy as np
    import bench
    from reina_model_amd import datasets, engine as eng, ensemble, simulation
    from reina_model_amd.variables import VARIABLE_DEFAULTS
    lib = eng.load_hip_library()
    m = describe(lib)
    n = int(float(a.agents)) if a.agents else int(agents)
    if a.group:
        windows = '0:60 60:125 125:365'
    wins = [tuple(int(x) for x in w.split(':')) for w in (a.windows or windows.split())]
    if n > 2_000_000 and not a.group:
        v, ages = bench.scaled_scenario(copy.deepcopy(VARIABLE_DEFAULTS), n)
    else:
        v, ages = copy.deepcopy(VARIABLE_DEFAULTS), datasets.get_population_for_area()
    ctx = simulation.make_context(v, age_counts=ages, seed=0)
    members = [simulation.make_context(v, age_counts=ages, seed=100 + k) for k in range(a.group)] if a.group else None
    shown = members[0] if members else ctx
    print('library %s: switches %s' % (os.path.basename(path), ' '.join(m['switches'])), flush=True)

    def mirror_of(c):
        return c.engine.alloc.to_host(c.engine.tensors['mirror']).view(np.uint64)

    def advance(days, timed=False):
        """so many days; timed: the kernels' us per launch from the HIP-event profile"""
        if members:
            ensemble.run_group_plan(members, ctx.make_plan(days))
            return {}
        if timed:
            ctx.engine.profile_enable(1)
            if a.what == 'ablate':
                ctx.engine.profile_read_kernels()
        ctx.run(days, record_history=a.what != 'ablate')
        ctx.synchronize()
        k = ctx.engine.profile_read_kernels() if timed else {}
        if timed:
            ctx.engine.profile_enable(0)
        return {name: ms * 1000 / c for name, (ms, c) in k.items() if c}

    day = 0
    if a.what == 'ablate':
        start = a.start if a.start is not None else int(os.environ.get('ABLATE_START', '92'))
        lib.reina_debug_ablate.argtypes = [ctypes.c_uint32]
        advance(start)
        for bits in a.bits or ['0']:
            assert lib.reina_debug_ablate(number_of(m['bit'], bits)) == 0
            ctx.engine.tensors['mirror'].zero_()
            k = advance(a.days, timed=True)
            print('ablate %s day %d: %s us | %s' % (bits, start, ' '.join('%s %.1f' % kv for kv in k.items()), window_line(m, mirror_of(ctx), a.days, a.raw)), flush=True)
            start += a.days
    else:
        for lo, hi in wins:
            if lo > day:
                advance(lo - day)
            for c in (members[:2] if members else [ctx]):
                c.engine.tensors['mirror'].zero_()
            k = advance(hi - lo, timed=a.what == 'prof')
            day = hi
            part = [name for name, number in m['part'].items() if number == m['prof']]
            head = 'days %3d-%3d' % (lo, hi) + (' part %s: k_day %.1f us' % (part[0], k.get('k_day', 0.0)) if a.what == 'prof' else '')
            print('%s | %s' % (head, window_line(m, mirror_of(shown), hi - lo, a.raw)), flush=True)
    sha = lambda name: hashlib.sha256(shown.engine.alloc.to_host(shown.engine.tensors[name]).tobytes()).hexdigest()  # noqa: E731
    print('sha256 hot %s counters %s' % (sha('hot'), sha('counters')), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = p.add_subparsers(dest='cmd', required=True)
    b = sub.add_parser('build')
    b.add_argument('switches', nargs='*')
    b.add_argument('--all', action='store_true')
    r = sub.add_parser('run')
    r.add_argument('what', choices=sorted(RUNS))
    r.add_argument('rest', nargs='*', help='[part (prof only)] [agents] [lo:hi ...]')
    r.add_argument('--group', type=int, default=0)
    r.add_argument('--wgs', type=int, default=0)
    r.add_argument('--start', type=int)
    r.add_argument('--days', type=int, default=3)
    r.add_argument('--bits', nargs='*')
    r.add_argument('--prof')
    r.add_argument('--lib', help='a variant built elsewhere')
    r.add_argument('--raw', action='store_true')
    a = p.parse_args()
    if a.cmd == 'build':
        todo = VARIANTS if a.all else [tuple(a.switches)]
        with concurrent.futures.ThreadPoolExecutor(max_workers=min(16, len(todo))) as pool:
            for path in pool.map(build, todo):
                print(path, flush=True)
        return
    rest = list(a.rest)
    if a.what == 'prof' and not rest:
        p.error('prof needs the number of a part')
    a.part = rest.pop(0) if a.what == 'prof' else None
    a.agents = rest.pop(0) if rest and ':' not in rest[0] else None
    a.windows = rest
    run(a)


if __name__ == '__main__':
    main()
