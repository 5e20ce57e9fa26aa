// reina_hip.hip part: per-member disease parameters of an engine group (include/reina_params.h; DESIGN.md section 6p).
// Included at the end of reina_hip.hip (it uses the host helpers, the group and the attachment base above); not a standalone header.
//
// ONE launch, k_group_params, expands the base disease and a member's theta into that member's parameter block: blockIdx.y =
// the position in the member list, one workgroup a member.  A thread owns cells of the fields a knob may scale (the 28
// per-variant scalars, then p_susceptibility and the five per-age arrays, which follow each other in reina_disease_t), reads
// the base cell, finds the knob that covers it and writes the member's cell; a cell no knob covers is not written.  The base
// and the knob table are read from the device copy through the constant address space; the member list and theta travel as
// the kernel argument.  The kernels of the next launch read the block through the scalar cache: the kernel boundary on the one
// stream stands between, as between k_group_tables and the day it precedes.
#include <cmath>

#include "../../include/reina_params.h"

#define PARAMS_THREADS 256
#define PARAMS_SCALAR_CELLS (7u * REINA_MAX_VARIANTS)                                   // fields 0..6, [field][variant]
#define PARAMS_SUS_CELLS ((uint32_t)REINA_MAX_VARIANTS * REINA_MAX_AGES)                // field 7, [variant][age]
#define PARAMS_CELLS (PARAMS_SCALAR_CELLS + PARAMS_SUS_CELLS + 5u * REINA_MAX_AGES)     // fields 8..12, [field][age]
#define PARAMS_SUS_WORD (offsetof(reina_disease_t, p_susceptibility) / 4u)
// the probabilities: the fields whose name begins with p_, but p_susceptibility -- a RELATIVE susceptibility (the default
// scenario's reaches 1.47), used only as p_susceptibility / psus_max and psus_max * multiplier: it is scaled and not clamped
#define PARAMS_CLAMPED (~(1u << REINA_PF_INFECTIOUSNESS_MULTIPLIER | 1u << REINA_PF_MEAN_INCUBATION_DURATION | \
                          1u << REINA_PF_MEAN_DURATION_FROM_ONSET_TO_DEATH | 1u << REINA_PF_MEAN_DURATION_FROM_ONSET_TO_RECOVERY | \
                          1u << REINA_PF_P_SUSCEPTIBILITY))
static_assert(offsetof(reina_disease_t, infectiousness_multiplier) == 0 && offsetof(reina_disease_t, p_asymptomatic_infection) == 16 &&
              offsetof(reina_disease_t, p_hospital_death_no_beds) == 32 && offsetof(reina_disease_t, p_icu_death_no_beds) == 48 &&
              offsetof(reina_disease_t, mean_incubation_duration) == 64 && offsetof(reina_disease_t, mean_duration_from_onset_to_death) == 80 &&
              offsetof(reina_disease_t, mean_duration_from_onset_to_recovery) == 96,
              "scalar cell c = field * REINA_MAX_VARIANTS + variant is float c of the block");
static_assert(offsetof(reina_disease_t, p_symptomatic) == offsetof(reina_disease_t, p_susceptibility) + 4u * PARAMS_SUS_CELLS &&
              offsetof(reina_disease_t, p_severe_given_symptomatic) == offsetof(reina_disease_t, p_symptomatic) + 4u * REINA_MAX_AGES &&
              offsetof(reina_disease_t, p_critical_given_severe) == offsetof(reina_disease_t, p_symptomatic) + 8u * REINA_MAX_AGES &&
              offsetof(reina_disease_t, p_fatal_given_critical) == offsetof(reina_disease_t, p_symptomatic) + 12u * REINA_MAX_AGES &&
              offsetof(reina_disease_t, p_death_outside_hospital) == offsetof(reina_disease_t, p_symptomatic) + 16u * REINA_MAX_AGES,
              "p_susceptibility and the five per-age arrays follow each other");
static_assert(REINA_MAX_VARIANTS == 4 && REINA_MAX_AGES == 128, "the cells' shifts");
static_assert(offsetof(DevParams, dis) == 0, "a member's disease block heads its parameter block");

// ---- the rule, once for the kernel and the host mirror

// cell c of [0, PARAMS_CELLS): its field, variant and age (0 where the field has none), and its float in reina_disease_t
struct ParamsCell { uint32_t field, v, a, word; };
__host__ __device__ static inline ParamsCell params_cell(uint32_t c) {
    ParamsCell x;
    if (c < PARAMS_SCALAR_CELLS) {
        x.field = c >> 2; x.v = c & 3u; x.a = 0u; x.word = c;
        return x;
    }
    const uint32_t k = c - PARAMS_SCALAR_CELLS;
    x.word = (uint32_t)PARAMS_SUS_WORD + k;
    x.a = k & 127u;
    if (k < PARAMS_SUS_CELLS) {
        x.field = REINA_PF_P_SUSCEPTIBILITY; x.v = k >> 7;
    } else {
        x.field = REINA_PF_P_SYMPTOMATIC + ((k - PARAMS_SUS_CELLS) >> 7); x.v = 0u;
    }
    return x;
}
__host__ __device__ static inline bool params_covers(uint32_t k_field, uint32_t k_variants, uint32_t k_lo, uint32_t k_hi, const ParamsCell &x) {
    if (k_field != x.field) return false;
    const bool v_ok = x.field > REINA_PF_P_SUSCEPTIBILITY || ((k_variants >> x.v) & 1u) != 0u;
    const bool a_ok = x.field < REINA_PF_P_SUSCEPTIBILITY || (x.a >= k_lo && x.a <= k_hi);
    return v_ok && a_ok;
}
// one float32 multiplication, one rounding; the probabilities clamped to 1
__host__ __device__ static inline float params_value(float base, float theta, uint32_t field) {
    const float r = base * theta;
    return ((PARAMS_CLAMPED >> field) & 1u) != 0u && r > 1.0f ? 1.0f : r;
}

// what the group keeps on the device: the base and the knob table
struct ParamsBlock {
    reina_disease_t base;
    reina_knob_t knobs[REINA_PARAMS_MAX_KNOBS];
};
struct ParamsArgs {
    uint32_t n_knobs, nr_ages, nr_variants;
    uint32_t sus_variants;                      // the variants a p_susceptibility knob covers: their psus_max is written
    uint32_t w[REINA_PARAMS_CHUNK_WORDS];       // per listed member: its index, then n_knobs theta (float bits)
};
static_assert(sizeof(ParamsArgs) + 2 * sizeof(void *) <= 3712u, "the kernel argument stays well inside 4 KiB");

// the new value of cell x for the theta at a.w[at ..], and whether a knob covers it: at most REINA_PARAMS_MAX_KNOBS compares, all
// of them on uniform values (the knob table and theta are scalar loads)
__device__ __forceinline__ bool params_new_value(const CAS ParamsBlock *blk, const ParamsArgs &a, uint32_t at, const ParamsCell &x, float *out) {
    const float b = reinterpret_cast<const CAS float *>(&blk->base)[x.word];
    bool covered = false;
    float th = 1.0f;
#pragma unroll
    for (uint32_t k = 0; k < REINA_PARAMS_MAX_KNOBS; k++) {
        if (k < a.n_knobs && params_covers(blk->knobs[k].field, blk->knobs[k].variants, blk->knobs[k].age_lo, blk->knobs[k].age_hi, x)) {
            covered = true;
            th = rp_u2f(a.w[at + k]);
        }
    }
    *out = covered ? params_value(b, th, x.field) : b;
    return covered;
}

__global__ __launch_bounds__(PARAMS_THREADS) void k_group_params(const MemberRef *M_, const ParamsBlock *blk_, const ParamsArgs a) {
    __shared__ float s_max[REINA_MAX_VARIANTS][2];
    const CAS ParamsBlock *blk = (const CAS ParamsBlock *)blk_;
    const uint32_t at = blockIdx.y * (1u + a.n_knobs);
    MemberRef ref;
    member_from_constant(&ref, M_ + a.w[at]);
    GAS float *dis = (GAS float *)const_cast<DevParams *>(ref.P);   // (DevParams.dis heads the block)
    for (uint32_t c = threadIdx.x; c < PARAMS_CELLS; c += PARAMS_THREADS) {
        const ParamsCell x = params_cell(c);
        float nv;
        if (params_new_value(blk, a, at + 1u, x, &nv)) dis[x.word] = nv;
    }
    if (a.sus_variants == 0u) return;   // (uniform)
    // psus_max of the variants a knob covers: thread = age (the first two waves; with 101 ages the second is partial: the lanes
    // past nr_ages bring 0.0f, where the maximum starts)
    if (threadIdx.x < REINA_MAX_AGES) {
        for (uint32_t v = 0; v < a.nr_variants; v++) {
            if (!((a.sus_variants >> v) & 1u)) continue;
            ParamsCell x;
            x.field = REINA_PF_P_SUSCEPTIBILITY; x.v = v; x.a = threadIdx.x;
            x.word = (uint32_t)PARAMS_SUS_WORD + v * REINA_MAX_AGES + threadIdx.x;
            float nv = 0.0f;
            if (threadIdx.x < a.nr_ages) (void)params_new_value(blk, a, at + 1u, x, &nv);
            float m = nv > 0.0f ? nv : 0.0f;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const float o = __shfl_xor(m, off);
                m = o > m ? o : m;
            }
            if ((threadIdx.x & 63u) == 0u) s_max[v][threadIdx.x >> 6] = m;
        }
    }
    __syncthreads();
    if (threadIdx.x < a.nr_variants && ((a.sus_variants >> threadIdx.x) & 1u)) {
        const float m0 = s_max[threadIdx.x][0], m1 = s_max[threadIdx.x][1];
        GAS float *pm = (GAS float *)const_cast<float *>(ref.P->psus_max);
        pm[threadIdx.x] = m1 > m0 ? m1 : m0;
    }
}

// ---- host side

struct reina_params {
    attachment a;
    ParamsBlock h_blk;
    ParamsBlock *d_blk = nullptr;
    uint32_t n_knobs = 0, sus_variants = 0;
    std::vector<uint32_t> cells;   // the covered cells: cell | knob << 16
    std::vector<uint8_t> seen;     // per member, reina_group_params_set's duplicate check
};

static const char *const params_field_names[REINA_PF_NR] = {
    "infectiousness_multiplier", "p_asymptomatic_infection", "p_hospital_death_no_beds", "p_icu_death_no_beds",
    "mean_incubation_duration", "mean_duration_from_onset_to_death", "mean_duration_from_onset_to_recovery", "p_susceptibility",
    "p_symptomatic", "p_severe_given_symptomatic", "p_critical_given_severe", "p_fatal_given_critical", "p_death_outside_hospital"};

// the host mirror of one member: the same cells, the same functions
static void params_expand_host(const reina_params *p, reina_engine_t *m, const float *theta) {
    float *dis = reinterpret_cast<float *>(&m->h_params.dis);
    const float *base = reinterpret_cast<const float *>(&p->h_blk.base);
    for (uint32_t ck : p->cells) {
        const ParamsCell x = params_cell(ck & 0xFFFFu);
        dis[x.word] = params_value(base[x.word], theta[ck >> 16], x.field);
    }
    for (uint32_t v = 0; v < m->cfg.nr_variants; v++) {
        if (!((p->sus_variants >> v) & 1u)) continue;
        float mx = 0.0f;
        for (uint32_t a = 0; a < m->cfg.nr_ages; a++)
            if (m->h_params.dis.p_susceptibility[v][a] > mx) mx = m->h_params.dis.p_susceptibility[v][a];
        m->h_params.psus_max[v] = mx;
    }
}

extern "C" {

int reina_params_version(void) { return REINA_PARAMS_VERSION; }

int reina_group_params_create(reina_group_t *g, const reina_disease_t *base, const reina_knob_t *knobs, uint32_t n_knobs, reina_params_t **out) {
    const std::string w("reina_group_params_create");
    if (!g || g->members.empty() || !out) return REINA_E_INVALID;
    if (!base || !knobs) return refuse(w + ": no base disease / no knob table");
    if (n_knobs == 0 || n_knobs > REINA_PARAMS_MAX_KNOBS) return refuse(w + ": n_knobs must be in [1, REINA_PARAMS_MAX_KNOBS]");
    if (int rc = attachment_check_members(g->members, "reina_group_params_create", "a shard's peers would have to be set with it")) return rc;
    const reina_engine_t *e0 = g->members[0];
    const uint32_t A = e0->cfg.nr_ages, V = e0->cfg.nr_variants;
    for (auto m : g->members)
        if (std::memcmp(&m->h_params.dis, base, sizeof(reina_disease_t)) != 0)
            return refuse(w + ": a member's disease is not the base, byte for byte");
    for (uint32_t k = 0; k < n_knobs; k++) {
        const reina_knob_t &kn = knobs[k];
        const std::string kw = w + ": knob " + std::to_string(k);
        if (kn.field >= REINA_PF_NR) return refuse(kw + ": unknown field");
        const bool per_variant = kn.field <= REINA_PF_P_SUSCEPTIBILITY, per_age = kn.field >= REINA_PF_P_SUSCEPTIBILITY;
        if (per_variant && kn.variants == 0u) return refuse(kw + " (" + params_field_names[kn.field] + "): no variant");
        if (per_variant && (kn.variants >> V) != 0u) return refuse(kw + " (" + params_field_names[kn.field] + "): a variant bit at or above nr_variants");
        if (!per_variant && kn.variants != 0u) return refuse(kw + " (" + params_field_names[kn.field] + "): a per-age field takes no variants");
        if (per_age && (kn.age_lo > kn.age_hi || kn.age_hi >= A)) return refuse(kw + " (" + params_field_names[kn.field] + "): the age range is reversed or outside [0, nr_ages)");
        if (!per_age && (kn.age_lo != 0u || kn.age_hi != 0u)) return refuse(kw + " (" + params_field_names[kn.field] + "): a per-variant scalar takes no ages");
    }
    std::vector<uint32_t> cells;
    uint32_t sus_variants = 0;
    const float *bw = reinterpret_cast<const float *>(base);
    for (uint32_t c = 0; c < PARAMS_CELLS; c++) {
        const ParamsCell x = params_cell(c);
        if (((PARAMS_CLAMPED >> x.field) & 1u) && !(bw[x.word] >= 0.0f && bw[x.word] <= 1.0f))
            return refuse(w + ": the base's " + params_field_names[x.field] + " has a value outside [0, 1]");
        if (x.field == REINA_PF_P_SUSCEPTIBILITY && (!(bw[x.word] >= 0.0f) || std::isinf(bw[x.word])))
            return refuse(w + ": the base's p_susceptibility has a value that is negative or not finite");
        int owner = -1;
        for (uint32_t k = 0; k < n_knobs; k++) {
            if (!params_covers(knobs[k].field, knobs[k].variants, knobs[k].age_lo, knobs[k].age_hi, x)) continue;
            if (owner >= 0) return refuse(w + ": knobs " + std::to_string(owner) + " and " + std::to_string(k) + " overlap (" + params_field_names[x.field] + ")");
            owner = (int)k;
        }
        if (owner >= 0) {
            cells.push_back(c | (uint32_t)owner << 16);
            if (x.field == REINA_PF_P_SUSCEPTIBILITY) sus_variants |= 1u << x.v;
        }
    }
    reina_params *p = new reina_params();
    p->a.e0 = g->members[0];
    p->a.g = g;
    p->a.members = g->members;
    p->a.d_refs = g->d_refs;
    std::memset(&p->h_blk, 0, sizeof(ParamsBlock));
    p->h_blk.base = *base;
    std::memcpy(p->h_blk.knobs, knobs, sizeof(reina_knob_t) * n_knobs);
    p->n_knobs = n_knobs;
    p->sus_variants = sus_variants;
    p->cells.swap(cells);
    p->seen.assign(g->members.size(), 0);
    HIP_CHECK_OR(hipMalloc(&p->d_blk, sizeof(ParamsBlock)), delete p);
    HIP_CHECK_OR(hipMemcpy(p->d_blk, &p->h_blk, sizeof(ParamsBlock), hipMemcpyHostToDevice), { (void)hipFree(p->d_blk); delete p; });
    *out = p;
    return REINA_OK;
}

int reina_group_params_destroy(reina_params_t *p) {
    if (!p) return REINA_E_INVALID;
    (void)hipFree(p->d_blk);
    delete p;
    return REINA_OK;
}

int reina_group_params_set(reina_params_t *p, const uint32_t *members, uint32_t n, const float *theta, void *stream) {
    if (!p) return REINA_E_INVALID;
    if (n == 0) return REINA_OK;
    const std::string w("reina_group_params_set");
    if (!members || !theta) return refuse(w + ": no member list / no theta");
    const uint32_t K = (uint32_t)p->a.members.size(), P = p->n_knobs;
    // every check before anything is queued: a refused call leaves every block, and every mirror, untouched
    int bad = 0;
    for (uint32_t j = 0; j < n && !bad; j++) {
        if (members[j] >= K) bad = 1;
        else if (p->seen[members[j]]) bad = 2;
        else p->seen[members[j]] = 1;
    }
    for (uint32_t j = 0; j < n; j++)
        if (members[j] < K) p->seen[members[j]] = 0;
    if (bad == 1) return refuse(w + ": a member index is out of range");
    if (bad == 2) return refuse(w + ": a member is listed twice");
    for (size_t k = 0; k < (size_t)n * P; k++)
        if (!(theta[k] >= 0.0f) || std::isinf(theta[k])) return refuse(w + ": theta must be finite and not negative");
    const reina_engine_t *e0 = p->a.e0;
    ParamsArgs a;
    a.n_knobs = P;
    a.nr_ages = e0->cfg.nr_ages;
    a.nr_variants = e0->cfg.nr_variants;
    a.sus_variants = p->sus_variants;
    const uint32_t chunk = REINA_PARAMS_CHUNK(P);
    for (uint32_t j0 = 0; j0 < n; j0 += chunk) {
        const uint32_t cn = n - j0 < chunk ? n - j0 : chunk;
        for (uint32_t j = 0; j < cn; j++) {
            a.w[j * (1u + P)] = members[j0 + j];
            std::memcpy(&a.w[j * (1u + P) + 1u], theta + (size_t)(j0 + j) * P, sizeof(float) * P);
        }
        hipLaunchKernelGGL(k_group_params, dim3(1, cn), dim3(PARAMS_THREADS), 0, (hipStream_t)stream, p->a.d_refs, p->d_blk, a);
        HIP_CHECK(hipGetLastError());
    }
    for (uint32_t j = 0; j < n; j++) params_expand_host(p, p->a.members[members[j]], theta + (size_t)j * P);
    return REINA_OK;
}

int reina_group_params_read(reina_params_t *p, uint32_t member, reina_disease_t *out, float *psus_max_out, void *stream) {
    if (!p) return REINA_E_INVALID;
    if (!out || !psus_max_out) return refuse("reina_group_params_read: no output");
    if (member >= p->a.members.size()) return refuse("reina_group_params_read: member out of range");
    const DevParams *d = p->a.members[member]->d_params;
    hipStream_t s = (hipStream_t)stream;
    HIP_CHECK(hipMemcpyAsync(out, &d->dis, sizeof(reina_disease_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(psus_max_out, d->psus_max, sizeof(float) * REINA_MAX_VARIANTS, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    return REINA_OK;
}

}  // extern "C"
