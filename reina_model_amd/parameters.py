"""Disease parameters per member of an engine group (include/reina_params.h; DESIGN.md section 6p "Parameters per particle").

A member carries a small vector theta of multipliers, one per Knob of a ParameterSpace; a knob scales one field of the disease
block (engine.Disease) on some of its cells.  expand_numpy is the executable specification of the rule the library applies
(reina_group_params_set: one launch for all listed members):

    a cell a knob covers      float32(base) * float32(theta), one rounding; the probabilities (CLAMPED: the fields whose name
                              begins with p_, but the relative p_susceptibility) are then clamped to 1
    a cell no knob covers     the base's
    psus_max[v]               the maximum over a < nr_ages of the new p_susceptibility[v][a], from 0

theta = 1 reproduces the base bit for bit; two knobs never cover one cell.  The module also holds the priors, the draw of a
prior table and the Liu-West step the particle filter perturbs theta with at a resample (filtering.particle_filter(...,
parameters=space)), and DeviceParameters, the handle of the device side.
"""
import ctypes
import math

import numpy as np

from . import engine as _eng

PARAMS_VERSION = 1              # include/reina_params.h: REINA_PARAMS_VERSION
MAX_KNOBS = 8                   # REINA_PARAMS_MAX_KNOBS
CHUNK_WORDS = 864               # REINA_PARAMS_CHUNK_WORDS
PARAMS_FUNCTIONS = ('params_version', 'group_params_create', 'group_params_destroy', 'group_params_set', 'group_params_read')
# REINA_PF_*: the fields a knob may scale, in the order of reina_disease_t
SCALAR_FIELDS = ('infectiousness_multiplier', 'p_asymptomatic_infection', 'p_hospital_death_no_beds', 'p_icu_death_no_beds',
                 'mean_incubation_duration', 'mean_duration_from_onset_to_death', 'mean_duration_from_onset_to_recovery')
AGE_FIELDS = ('p_symptomatic', 'p_severe_given_symptomatic', 'p_critical_given_severe', 'p_fatal_given_critical',
              'p_death_outside_hospital')
FIELDS = SCALAR_FIELDS + ('p_susceptibility',) + AGE_FIELDS
# the probabilities, clamped to 1: the p_ fields but p_susceptibility, a RELATIVE susceptibility (the default scenario's reaches
# 1.47; the engine uses it as p_susceptibility / psus_max and psus_max * multiplier), which is scaled and not clamped
CLAMPED = tuple(f for f in FIELDS if f.startswith('p_') and f != 'p_susceptibility')


def chunk(n_knobs):
    """members one launch of reina_group_params_set serves (REINA_PARAMS_CHUNK)"""
    return CHUNK_WORDS // (1 + int(n_knobs))


class KnobABI(ctypes.Structure):
    _fields_ = [('field', ctypes.c_uint32), ('variants', ctypes.c_uint32), ('age_lo', ctypes.c_uint32), ('age_hi', ctypes.c_uint32)]


def bind_params_abi(lib, prefix):
    """The per-member parameter entry points of a library (include/reina_params.h), or None when it has none."""
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    argtypes = {'group_params_create': [vp, vp, vp, u32, vp], 'group_params_destroy': [vp],
                'group_params_set': [vp, vp, u32, vp, vp], 'group_params_read': [vp, u32, vp, vp, vp]}
    return _eng.bind_optional_abi(lib, prefix, PARAMS_FUNCTIONS, argtypes, 'params_version', PARAMS_VERSION)


# ------------------------------------------------------------------------------------------------ priors

class LogNormal:
    """theta = median * exp(sigma * z), z standard normal"""
    uniform = False

    def __init__(self, median, sigma):
        if not (float(median) > 0 and math.isfinite(float(median)) and float(sigma) >= 0 and math.isfinite(float(sigma))):
            raise ValueError('LogNormal: median must be positive and sigma not negative')
        self.median, self.sigma = float(median), float(sigma)

    def draw(self, z):
        return self.median * np.exp(self.sigma * np.asarray(z, dtype=np.float64))

    def quantile(self, q):
        from statistics import NormalDist
        return self.median * math.exp(self.sigma * NormalDist().inv_cdf(float(q)))


class Uniform:
    """theta = lo + (hi - lo) * u, u uniform in [0, 1)"""
    uniform = True

    def __init__(self, lo, hi):
        if not (0 < float(lo) <= float(hi) and math.isfinite(float(hi))):
            raise ValueError('Uniform: 0 < lo <= hi')
        self.lo, self.hi = float(lo), float(hi)

    def draw(self, u):
        return self.lo + (self.hi - self.lo) * np.asarray(u, dtype=np.float64)

    def quantile(self, q):
        return self.lo + (self.hi - self.lo) * float(q)


class Fixed:
    """theta = value for every member, at every resample"""
    uniform = False

    def __init__(self, value):
        if not (float(value) >= 0 and math.isfinite(float(value))):
            raise ValueError('Fixed: a finite value that is not negative')
        self.value = float(value)

    def draw(self, z):
        return np.full(np.shape(z), self.value, dtype=np.float64)

    def quantile(self, q):
        return self.value


class Knob:
    """One multiplier: `field` (one of FIELDS) scaled on `variants` (indices, 0 = wild-type; None: all; per-variant fields and
    p_susceptibility only) and `ages` ((lo, hi) inclusive; None: all; p_susceptibility and the per-age fields only).  `prior`: a
    LogNormal, Uniform or Fixed (default Fixed(1.0)); `bounds` (lo, hi) with 0 < lo <= hi: a drawn or perturbed theta is clipped
    to them (a Fixed knob keeps its value whatever they are)."""

    def __init__(self, name, field, variants=None, ages=None, prior=None, bounds=(1e-3, 1e3)):
        self.name = str(name)
        self.field = field
        self.variants = None if variants is None else tuple(int(v) for v in variants)
        self.ages = None if ages is None else (int(ages[0]), int(ages[1]))
        self.prior = Fixed(1.0) if prior is None else prior
        if not isinstance(self.prior, (LogNormal, Uniform, Fixed)):
            raise ValueError('knob %r: the prior is a LogNormal, a Uniform or a Fixed' % self.name)
        lo, hi = float(bounds[0]), float(bounds[1])
        if not (0 < lo <= hi and math.isfinite(hi)):
            raise ValueError('knob %r: bounds are (lo, hi) with 0 < lo <= hi' % self.name)
        self.bounds = (lo, hi)

    @property
    def fixed(self):
        return isinstance(self.prior, Fixed)


class ParameterSpace:
    """The knobs of one inference, in the order of theta's columns.  Refused here (ValueError), as by reina_group_params_create:
    no knob or more than MAX_KNOBS, an unknown field, variants on a per-age field, ages on a per-variant scalar, an empty list
    of variants, a reversed or negative age range, two knobs that cover a common cell; names must differ.  check(nr_ages,
    nr_variants) refuses what needs the population: ages at or above nr_ages, variants at or above nr_variants."""

    def __init__(self, knobs):
        self.knobs = list(knobs)
        if not 1 <= len(self.knobs) <= MAX_KNOBS:
            raise ValueError('ParameterSpace: between 1 and %d knobs' % MAX_KNOBS)
        if len(set(k.name for k in self.knobs)) != len(self.knobs):
            raise ValueError('ParameterSpace: two knobs share a name')
        for k in self.knobs:
            if k.field not in FIELDS:
                raise ValueError('knob %r: unknown field %r (have %s)' % (k.name, k.field, ', '.join(FIELDS)))
            if k.field in AGE_FIELDS and k.variants is not None:
                raise ValueError('knob %r: %s is a per-age field and takes no variants' % (k.name, k.field))
            if k.field in SCALAR_FIELDS and k.ages is not None:
                raise ValueError('knob %r: %s is a per-variant scalar and takes no ages' % (k.name, k.field))
            if k.variants is not None and (not k.variants or min(k.variants) < 0):
                raise ValueError('knob %r: variants are indices in [0, nr_variants), at least one' % k.name)
            if k.ages is not None and not 0 <= k.ages[0] <= k.ages[1]:
                raise ValueError('knob %r: the age range is reversed or negative' % k.name)
        self.table(_eng.MAX_AGES, _eng.MAX_VARIANTS, _limits=False)

    def __len__(self):
        return len(self.knobs)

    @property
    def names(self):
        return [k.name for k in self.knobs]

    def index(self, name):
        if name not in self.names:
            raise ValueError('no knob %r (have %s)' % (name, ', '.join(self.names)))
        return self.names.index(name)

    def table(self, nr_ages, nr_variants, _limits=True):
        """[(field index, variant mask, age_lo, age_hi)] of the knobs for a population: reina_knob_t's words"""
        rows = []
        for k in self.knobs:
            f = FIELDS.index(k.field)
            if _limits and k.variants is not None and max(k.variants) >= nr_variants:
                raise ValueError('knob %r: a variant at or above nr_variants (%d)' % (k.name, nr_variants))
            if _limits and k.ages is not None and k.ages[1] >= nr_ages:
                raise ValueError('knob %r: the age range is outside [0, nr_ages) (%d)' % (k.name, nr_ages))
            mask = 0
            if k.field not in AGE_FIELDS:
                for v in (range(nr_variants) if k.variants is None else k.variants):
                    mask |= 1 << v
            lo, hi = (0, 0) if k.field in SCALAR_FIELDS else ((0, nr_ages - 1) if k.ages is None else k.ages)
            rows.append((f, mask, lo, hi))
        for i, a in enumerate(rows):
            for j in range(i):
                b = rows[j]
                if a[0] != b[0]:
                    continue
                shared_v = a[0] > len(SCALAR_FIELDS) or (a[1] & b[1]) != 0
                shared_a = a[0] < len(SCALAR_FIELDS) or (a[2] <= b[3] and b[2] <= a[3])
                if shared_v and shared_a:
                    raise ValueError('knobs %r and %r overlap (%s)' % (self.knobs[j].name, self.knobs[i].name, FIELDS[a[0]]))
        return rows

    def check(self, nr_ages, nr_variants):
        self.table(nr_ages, nr_variants)

    # ---- theta of a filter: the state is log theta; theta is what the engine is handed

    def theta_of(self, log_theta):
        """theta [K, P] (float64 holding float32 values: what the device is handed) of log theta: exp, clipped to the knobs'
        bounds; a Fixed knob's column is its value"""
        lt = np.asarray(log_theta, dtype=np.float64)
        th = np.exp(lt)
        for p, k in enumerate(self.knobs):
            th[..., p] = k.prior.value if k.fixed else np.clip(th[..., p], k.bounds[0], k.bounds[1])
        return th.astype(np.float32).astype(np.float64)

    def draw_prior(self, n, gen):
        """log theta [n, P] of the prior: n x P draws of `gen` in C order, a standard normal per cell (a uniform for the cells of
        a Uniform prior; a Fixed knob's draw is taken and not used, so that the stream does not depend on the priors' kinds)"""
        P = len(self.knobs)
        if any(k.prior.uniform for k in self.knobs):
            z = np.array([[gen.random() if k.prior.uniform else gen.standard_normal() for k in self.knobs] for _ in range(n)],
                         dtype=np.float64).reshape(n, P)
        else:
            z = gen.standard_normal((n, P))
        lt = np.zeros((n, P), dtype=np.float64)
        for p, k in enumerate(self.knobs):
            if k.fixed:
                lt[:, p] = math.log(k.prior.value) if k.prior.value > 0 else -math.inf
            else:
                lt[:, p] = np.clip(np.log(k.prior.draw(z[:, p])), math.log(k.bounds[0]), math.log(k.bounds[1]))
        return lt

    def liu_west(self, log_theta, weights, ancestors, z, shrinkage):
        """The Liu-West kernel-shrinkage step of a resample, in log theta: with delta = shrinkage, a = (3 delta - 1) / (2 delta)
        and h^2 = 1 - a^2, per knob m = sum_i w_i log theta_i, s^2 = sum_i w_i (log theta_i - m)^2 under the pre-resample weights,
        and log theta'_k = a log theta_anc[k] + (1 - a) m + h s z_k, clipped to the knob's bounds.  Fixed knobs and knobs with
        s = 0 take their ancestor's value unchanged.  z: [K, P] standard normals."""
        lt = np.asarray(log_theta, dtype=np.float64)
        w = np.asarray(weights, dtype=np.float64)
        anc = np.asarray(ancestors, dtype=np.int64)
        z = np.asarray(z, dtype=np.float64)
        d = float(shrinkage)
        if not 0.5 < d <= 1.0:
            raise ValueError('liu_west: shrinkage is in (0.5, 1]')
        a = (3.0 * d - 1.0) / (2.0 * d)
        h = math.sqrt(max(1.0 - a * a, 0.0))
        out = lt[anc].copy()
        for p, k in enumerate(self.knobs):
            if k.fixed:
                continue
            m = float(np.sum(w * lt[:, p]))
            s = math.sqrt(max(float(np.sum(w * (lt[:, p] - m) ** 2)), 0.0))
            if s == 0.0:
                continue
            out[:, p] = np.clip(a * lt[anc, p] + (1.0 - a) * m + h * s * z[:, p], math.log(k.bounds[0]), math.log(k.bounds[1]))
        return out


# ------------------------------------------------------------------------------------------------ the rule in numpy

def _copy_disease(d):
    out = _eng.Disease()
    ctypes.memmove(ctypes.byref(out), ctypes.byref(d), ctypes.sizeof(_eng.Disease))
    return out


def disease_bytes(d):
    return ctypes.string_at(ctypes.byref(d), ctypes.sizeof(_eng.Disease))


def psus_max_of(disease, nr_ages, nr_variants):
    """psus_max [MAX_VARIANTS] float32 as reina_create computes it: per variant the maximum over a < nr_ages, from 0"""
    sus = np.ctypeslib.as_array(disease.p_susceptibility)
    out = np.zeros(_eng.MAX_VARIANTS, dtype=np.float32)
    for v in range(nr_variants):
        m = np.float32(0.0)
        for x in sus[v, :nr_ages]:
            if x > m:
                m = x
        out[v] = m
    return out


def expand_numpy(base_disease, space, theta, nr_ages, nr_variants):
    """(engine.Disease, psus_max float32 [MAX_VARIANTS]) of one member: the base with every cell a knob covers multiplied by the
    knob's theta in float32 and, for the probabilities (CLAMPED), clamped to 1.  Refuses what reina_group_params_create and _set refuse of
    knobs, base and theta."""
    d = expand_many(base_disease, space, np.asarray(theta, dtype=np.float32).reshape(1, -1), nr_ages, nr_variants)[0]
    return d, psus_max_of(d, nr_ages, nr_variants)


def expand_many(base_disease, space, thetas, nr_ages, nr_variants):
    """[engine.Disease] of the members of `thetas` [K, P]: expand_numpy's rule for all rows at once"""
    rows = space.table(nr_ages, nr_variants)
    th = np.asarray(thetas, dtype=np.float32)
    if th.ndim != 2 or th.shape[1] != len(rows):
        raise ValueError('expand_numpy: one theta per knob')
    if not np.all(np.isfinite(th) & (th >= 0)):
        raise ValueError('expand_numpy: theta must be finite and not negative')
    for name in CLAMPED:
        b = np.ctypeslib.as_array(getattr(base_disease, name))
        if not np.all((b >= 0) & (b <= 1)):
            raise ValueError('expand_numpy: the base has a %s outside [0, 1]' % name)
    b = np.ctypeslib.as_array(base_disease.p_susceptibility)
    if not np.all((b >= 0) & np.isfinite(b)):
        raise ValueError('expand_numpy: the base has a p_susceptibility outside [0, inf)')
    out = np.tile(np.frombuffer(disease_bytes(base_disease), dtype=np.float32), (len(th), 1))   # (the knobs' fields are floats)
    one = np.float32(1.0)
    for p, (f, mask, lo, hi) in enumerate(rows):
        name = FIELDS[f]
        word0 = getattr(_eng.Disease, name).offset // 4
        if name in SCALAR_FIELDS:
            idx = [word0 + v for v in range(_eng.MAX_VARIANTS) if mask >> v & 1]
        elif name in AGE_FIELDS:
            idx = [word0 + a for a in range(lo, hi + 1)]
        else:
            idx = [word0 + v * _eng.MAX_AGES + a for v in range(_eng.MAX_VARIANTS) if mask >> v & 1 for a in range(lo, hi + 1)]
        new = out[:, idx] * th[:, p:p + 1]   # float32 * float32: one multiplication, one rounding
        if name in CLAMPED:
            new = np.minimum(new, one)
        out[:, idx] = new
    return [_eng.Disease.from_buffer_copy(out[k].tobytes()) for k in range(len(th))]


# ------------------------------------------------------------------------------------------------ the device side

class DeviceParameters(_eng.Handle):
    """The reina_params_t of an engine group: `base` (engine.Disease, every member's current disease) and the knobs of `space`.
    set(members, theta) queues one expansion for the listed members; read(member) is the member's DEVICE block.  Close it before
    the group."""
    DESTROY = 'group_params_destroy'

    def __init__(self, group, base, space):
        from . import reports as _rep
        e0 = group.engines[0]
        self.f = _rep.entry_points(e0, 'params_f', 'per-member parameter', 'reina_params.h')
        self.group, self.space, self.e0 = group, space, e0
        self.base = _copy_disease(base)
        self.nr_ages, self.nr_variants = int(e0.config.nr_ages), int(e0.config.nr_variants)
        rows = space.table(self.nr_ages, self.nr_variants)
        knobs = (KnobABI * len(rows))(*[KnobABI(*r) for r in rows])
        self._h = ctypes.c_void_p()
        e0._check(self.f['group_params_create'](group._h, ctypes.byref(self.base), knobs, len(rows), ctypes.byref(self._h)),
                  'group_params_create')

    def set(self, members, theta):
        """member members[j] gets theta[j] ([n, P]): one call, chunk(P) members a launch, no host wait"""
        mem = np.ascontiguousarray(np.asarray(members, dtype=np.int64).reshape(-1))
        if len(mem) and (mem.min() < 0 or mem.max() > 0xFFFFFFFF):
            raise ValueError('params_set: a member index is out of range')
        mem = mem.astype(np.uint32)
        th = np.ascontiguousarray(np.asarray(theta, dtype=np.float32).reshape(len(mem), len(self.space)))
        _eng.mark_stale(self.group.engines)
        self.e0._check(self.f['group_params_set'](self._h, mem.ctypes.data, len(mem), th.ctypes.data, self.e0.alloc.stream()),
                       'group_params_set')

    def read(self, member):
        """(engine.Disease, psus_max float32 [MAX_VARIANTS]) as the device holds them; waits for the stream"""
        d = _eng.Disease()
        pm = np.zeros(_eng.MAX_VARIANTS, dtype=np.float32)
        self.e0._check(self.f['group_params_read'](self._h, int(member) & 0xFFFFFFFF, ctypes.byref(d), pm.ctypes.data,
                                                   self.e0.alloc.stream()), 'group_params_read')
        return d, pm

    def expand(self, theta):
        """expand_numpy of this handle's base and space"""
        return expand_numpy(self.base, self.space, theta, self.nr_ages, self.nr_variants)

    def expand_many(self, thetas):
        return expand_many(self.base, self.space, thetas, self.nr_ages, self.nr_variants)
