"""Build the HIP engine in-tree: `python -m reina_model_amd.build` -> csrc/libreina_hip.so.

hipcc cross-compiles gfx950 without a GPU.  FP contraction is OFF: the engine's integer results
must be bit-identical to the CPU checker, which needs the same rounding sequence on both sides."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
LIB = os.path.join(CSRC, 'libreina_hip.so')
SOURCES = [os.path.join(CSRC, 'reina_hip.hip')]
DEPS = SOURCES + [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith(('.inc', '.h'))] + [
                  os.path.join(os.path.dirname(HERE), 'include', 'reina_hip.h'),
                  os.path.join(os.path.dirname(HERE), 'include', 'reina_snapshot.h'),
                  os.path.join(os.path.dirname(HERE), 'include', 'reina_transmission.h'),
                  os.path.join(os.path.dirname(HERE), 'include', 'reina_filter.h'),
                  os.path.join(os.path.dirname(HERE), 'include', 'reina_filter_log.h'),
                  os.path.join(os.path.dirname(HERE), 'include', 'reina_policy.h'),
                  os.path.join(os.path.dirname(HERE), 'include', 'reina_txlog.h'),
                  os.path.join(os.path.dirname(HERE), 'include', 'reina_course.h'),
                  os.path.join(os.path.dirname(HERE), 'include', 'reina_vaccination.h'),
                  os.path.join(os.path.dirname(HERE), 'include', 'reina_detection.h'),
                  os.path.join(os.path.dirname(HERE), 'include', 'reina_regime.h'),
                  os.path.join(os.path.dirname(HERE), 'include', 'reina_lineage.h'),
                  os.path.join(os.path.dirname(HERE), 'include', 'reina_summary.h'),
                  os.path.join(os.path.dirname(HERE), 'include', 'reina_params.h')]
HIPCC_FLAGS = ['--offload-arch=gfx950', '-O3', '-fPIC', '-shared', '-std=c++17', '-ffp-contract=off',
               '-fno-fast-math']


def hipcc_path():
    for c in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc', 'hipcc'):
        if c and (os.path.sep not in c or os.path.exists(c)):
            return c
    return 'hipcc'


def build(force=False, verbose=False):
    if (not force and os.path.exists(LIB)
            and all(os.path.getmtime(LIB) >= os.path.getmtime(d) for d in DEPS)):
        return LIB
    cmd = [hipcc_path()] + HIPCC_FLAGS + ['-o', LIB] + SOURCES
    if verbose:
        print(' '.join(cmd))
    subprocess.run(cmd, check=True)
    return LIB


def build_variant(defines, out_path, verbose=False):
    """A diagnostic or code variant of the library: build()'s flags plus one -D per entry of `defines` ('REINA_OPEN_STAMPS',
    'REINA_DAY_PROF=9', ...), written to the side file `out_path` (selected at run time by REINA_HIP_LIB)."""
    out_path = os.path.abspath(out_path)
    if out_path == os.path.abspath(LIB):
        raise ValueError('a variant is a side file: %s is the production library' % LIB)
    cmd = [hipcc_path()] + HIPCC_FLAGS + ['-D' + d for d in defines] + ['-o', out_path] + SOURCES
    if verbose:
        print(' '.join(cmd))
    subprocess.run(cmd, check=True)
    return out_path


if __name__ == '__main__':
    build(force='--force' in sys.argv, verbose=True)
    print(LIB)
