/* oracle/reina_par.c -- TEST INFRASTRUCTURE (oracle "B"), never linked into the product.
 *
 * Plain-C, single-threaded restatement of the PARALLEL formulation of the reference's day step
 * (SURVEY.md Appendix B): the same model as cythonsim/main.pyx, reorganised into order-free
 * phases (imports -> test queue/tracing/vaccination -> scan -> hospital -> contacts -> install)
 * with every random decision keyed by (agent, day, purpose) on Philox instead of the reference's
 * sequential PCG64 stream.  The HIP engine must reproduce this program's integer state
 * BIT-EXACTLY (tests/test_parity_gpu.py); this program is tied to the reference statistically
 * (ensemble tolerance vs the bit-exact sequential oracle A, tests/test_par_vs_seq.py) because a
 * parallel engine cannot replay the PCG64 stream order.
 *
 * Written independently of the kernels (simple loops, arrays, qsort); it shares only the numeric
 * primitives header (Philox, reproducible exp/log/normal/gamma, hot-word bit layout) and the ABI
 * structs.  Exposes the engine ABI of include/reina_hip.h with a `par_` prefix and host memory.
 */
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/reina_hip.h"
#include "../reina_model_amd/csrc/reina_prims.h"
#include "../reina_model_amd/csrc/reina_sample.h"
#include "../reina_model_amd/csrc/reina_contacts.h"

typedef struct {
    reina_config_t cfg;
    reina_disease_t dis;
    reina_buffers_t buf;
    int bound;
    uint32_t k0, k1;
    /* contact tables (copied) */
    float nrc[REINA_MAX_AGES];
    int32_t tcount[REINA_MAX_AGES];
    uint32_t thr[REINA_MAX_AGES][REINA_MAX_ENTRIES];
    uint32_t meta[REINA_MAX_AGES][REINA_MAX_ENTRIES];
    float mask_p[REINA_MAX_AGES][8];
    uint32_t n_ranges;
    int32_t range_min[REINA_MAX_RANGES], range_max[REINA_MAX_RANGES];
    float psus_max[REINA_MAX_VARIANTS];
    uint32_t cthr[REINA_MAX_AGES][REINA_COUNT_WORDS];   /* contact-count thresholds of every age (reina_contacts.h) */
    uint32_t hosp_ranges, hosp_range_bits;              /* priority buckets of the day's bed / ICU events (sharded: exchanged maps) */
    reina_allreduce_fn coll_fn;
    void *coll_comm;
    /* exact cross-shard attribution (include/reina_hip.h): global ids in every link field, 8-byte records exchanged */
    int exact;
    uint32_t gid_base, gid_mask;   /* reina_prims.h: rp_gid_is_local */
    int32_t shard_age_start[REINA_MAX_SHARDS][REINA_MAX_AGES + 1];   /* every shard's age_start: a source works out its target's age */
    uint32_t shard_k0[REINA_MAX_SHARDS], shard_k1[REINA_MAX_SHARDS];  /* every shard's Philox key: a target recomputes its source's priority */
    reina_alltoall_fn a2a_fn;
    void *a2a_comm;
} Par;

#define CNT(e, c, age) ((e)->buf.counters[(c) * REINA_MAX_AGES + (age)])
#define SC(e, s) ((e)->buf.counters[REINA_C_NR * REINA_MAX_AGES + (s)])
#define CTL(e, l) ((e)->buf.control[(l)])

enum { EV_HOSPITALIZE = 0, EV_TO_ICU = 1, EV_RELEASE_WARD = 2, EV_RELEASE_ICU = 3 };

static void set_problem(Par *e, int p) {
    if (SC(e, REINA_S_PROBLEM) == 0) SC(e, REINA_S_PROBLEM) = p;
}

/* age of sorted agent index i (Population.age_start, main.pyx:1442) */
static int age_of(const Par *e, uint32_t i) {
    int lo = 0, hi = (int)e->cfg.nr_ages - 1;
    while (lo < hi) {
        int mid = (lo + hi + 1) >> 1;
        if ((uint32_t)e->cfg.age_start[mid] <= i)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

int par_abi_version(void) { return 7; }

/* ---------------------------------------------------------------- exact attribution: ids and exchange segments */
static int32_t gid_of(const Par *e, uint32_t i) { return (int32_t)(e->gid_base | i); }
static int gid_local(const Par *e, int32_t g) { return (int)rp_gid_is_local((uint32_t)g, e->gid_base, e->gid_mask); }
static uint32_t gid_index(const Par *e, int32_t g) { return (uint32_t)g & e->gid_mask; }
static uint64_t *xseg(const Par *e, uint64_t *buf, uint32_t shard) { return buf + (size_t)shard * REINA_XCHG_SEG_WORDS(e->cfg.xchg_cap, e->hosp_ranges); }
/* the trailer of a segment: what rides behind the records of the mid-day exchange (include/reina_hip.h: REINA_XCHG_TRAILER_WORDS) */
static uint64_t *xtrailer(const Par *e, uint64_t *buf, uint32_t shard) { return xseg(e, buf, shard) + 1u + e->cfg.xchg_cap; }
static void xsend_push(Par *e, uint32_t dest, uint64_t rec) {
    uint64_t *seg = xseg(e, e->buf.xsend, dest);
    if (seg[0] >= e->cfg.xchg_cap) {
        set_problem(e, REINA_PROBLEM_EXCHANGE_OVERFLOW);
        return;
    }
    seg[1 + seg[0]++] = rec;
}
static void xsend_reset(Par *e) {
    for (uint32_t sh = 0; sh < e->cfg.n_shards; sh++) {
        uint64_t *seg = xseg(e, e->buf.xsend, sh);
        if ((int64_t)seg[0] > CTL(e, REINA_L_XCHG_PEAK)) CTL(e, REINA_L_XCHG_PEAK) = (int32_t)seg[0];
        seg[0] = 0;
    }
}
/* records shard `sh` sent to this one in the last exchange */
static uint32_t xrecv_count(const Par *e, uint32_t sh) {
    const uint64_t n = xseg(e, e->buf.xrecv, sh)[0];
    return n > e->cfg.xchg_cap ? e->cfg.xchg_cap : (uint32_t)n;
}

/* Context.sample: the shared host-side sampler (utility, not part of the day step) */
int par_sample(const reina_disease_t *disease, uint64_t seed, int what, int age, int severity,
               float nr_contacts_of_age, int n, int32_t *out) {
    return reina_sample_impl(disease, seed, what, age, severity, nr_contacts_of_age, n, out);
}

/* the shared host-side contact-table build (utility, not part of the day step) */
int par_build_contact_tables(const double *base, const int32_t *row_page, const int32_t *row_place, uint32_t n_rows,
                             const double *mobility, uint32_t n_mobility, const int32_t *rows_mat,
                             const int32_t *sorted_mat, uint32_t n_ages, uint32_t n_entries, double *totals_out,
                             double *cum_out, float *nrc_out, uint32_t *thr_out, uint32_t thr_stride) {
    const int rc = reina_build_contact_tables_impl(base, row_page, row_place, n_rows, mobility, n_mobility, rows_mat, sorted_mat,
                                                   n_ages, n_entries, totals_out, cum_out, nrc_out, thr_out, thr_stride);
    return rc == 0 ? REINA_OK : REINA_E_INVALID;
}

int par_create(const reina_config_t *cfg, const reina_disease_t *disease, Par **out) {
    if (cfg->nr_ages > REINA_MAX_AGES || cfg->nr_variants > REINA_MAX_VARIANTS) return REINA_E_INVALID;
    Par *e = (Par *)calloc(1, sizeof(Par));
    e->cfg = *cfg;
    e->dis = *disease;
    if (e->cfg.n_shards == 0) e->cfg.n_shards = 1;
    if (e->cfg.n_shards > REINA_MAX_SHARDS || e->cfg.shard_rank >= e->cfg.n_shards) {
        free(e);
        return REINA_E_INVALID;
    }
    e->hosp_ranges = cfg->hosp_ranges ? cfg->hosp_ranges : REINA_HOSP_RANGES(cfg->n_agents);
    while ((1u << e->hosp_range_bits) < e->hosp_ranges) e->hosp_range_bits++;
    uint64_t seed = rp_shard_seed(cfg->seed, e->cfg.shard_rank);
    e->k0 = (uint32_t)seed;
    e->k1 = (uint32_t)(seed >> 32);
    for (uint32_t v = 0; v < cfg->nr_variants; v++) {
        float m = 0.0f;
        for (uint32_t a = 0; a < cfg->nr_ages; a++)
            if (disease->p_susceptibility[v][a] > m) m = disease->p_susceptibility[v][a];
        e->psus_max[v] = m;
    }
    e->exact = cfg->exact_attribution && e->cfg.n_shards > 1;
    e->gid_mask = 0xFFFFFFFFu;
    if (e->exact) {
        if (!cfg->shard_age_start || !cfg->xchg_cap || !cfg->pool_cap || cfg->n_agents > RP_GID_INDEX_MASK) {
            free(e);
            return REINA_E_INVALID;
        }
        e->gid_base = e->cfg.shard_rank << RP_GID_SHIFT;
        e->gid_mask = RP_GID_INDEX_MASK;
        memcpy(e->shard_age_start, cfg->shard_age_start, sizeof(int32_t) * (size_t)e->cfg.n_shards * (REINA_MAX_AGES + 1));
        for (uint32_t sh = 0; sh < e->cfg.n_shards; sh++) {
            const uint64_t ss = rp_shard_seed(cfg->seed, sh);
            e->shard_k0[sh] = (uint32_t)ss;
            e->shard_k1[sh] = (uint32_t)(ss >> 32);
        }
    }
    e->cfg.shard_age_start = NULL;   /* (the caller's array is not kept) */
    *out = e;
    return 0;
}
int par_destroy(Par *e) {
    free(e);
    return 0;
}
int par_bind_buffers(Par *e, const reina_buffers_t *b) {
    e->buf = *b;
    e->bound = 1;
    return 0;
}

/* _create_agents / _init_stats (main.pyx:1389-1450): everyone susceptible */
int par_init_state(Par *e, int32_t beds, int32_t icu, void *stream) {
    (void)stream;
    if (!e->bound) return REINA_E_NOT_BOUND;
    uint32_t N = e->cfg.n_agents;
    for (uint32_t i = 0; i < N; i++) {
        e->buf.hot[i] = 0;
        e->buf.cold[i].infector = -1;
        e->buf.cold[i].n_infected = 0;
        e->buf.cold[i].onset_days = 0.0f;
        e->buf.cold[i].vacc_day = -1;
        e->buf.cold[i].first_infectee = -1;
        e->buf.cold[i].next_sibling = -1;
        e->buf.cold[i].claim = ~0ull;
        for (int k = 0; k < REINA_INLINE_INFECTEES; k++) e->buf.infectees[(size_t)i * REINA_INLINE_INFECTEES + k] = -1;
    }
    if (e->cfg.n_shards > 1)
        for (size_t k = 0; k < (size_t)REINA_MAX_RANGES * REINA_MAX_VARIANTS * e->cfg.mirror_slots; k++)
            e->buf.mirror[k] = ~0ull;
    for (uint32_t c = 0; c < REINA_MIRROR_CELLS; c++) {   /* smallest tables, no entries yet */
        e->buf.mirror_meta[c] = e->cfg.mirror_slots < RP_MIRROR_MIN_SLOTS ? e->cfg.mirror_slots : RP_MIRROR_MIN_SLOTS;
        e->buf.mirror_meta[REINA_MIRROR_CELLS + c] = 0;
    }
    memset(e->buf.counters, 0, sizeof(int32_t) * REINA_COUNTER_WORDS);
    memset(e->buf.control, 0, sizeof(int32_t) * REINA_L_NR);
    if (e->exact) xsend_reset(e);
    for (uint32_t a = 0; a < e->cfg.nr_ages; a++)
        CNT(e, REINA_C_SUSCEPTIBLE, a) = e->cfg.age_start[a + 1] - e->cfg.age_start[a];
    SC(e, REINA_S_AVAILABLE_BEDS) = SC(e, REINA_S_BEDS) = beds;
    SC(e, REINA_S_AVAILABLE_ICU) = SC(e, REINA_S_ICU_UNITS) = icu;
    for (int k = 0; k < REINA_MAX_VACCINATIONS; k++) CTL(e, REINA_L_VACC_CURSOR + k) = INT_MIN;
    return 0;
}

static char g_par_error[128];   /* text of the last refusal (par_last_error) */
int par_upload_contact_tables(Par *e, const reina_contact_tables_t *t, void *stream) {
    (void)stream;
    uint32_t A = e->cfg.nr_ages;
    for (uint32_t a = 0; a < A; a++)
        if (t->count[a] == 0 && t->nr_contacts_by_age[a] > 0.0f) {   /* (run_contacts would index entry -1 of an empty row) */
            snprintf(g_par_error, sizeof(g_par_error),
                     "age %u has contacts (nr_contacts_by_age > 0) but no contact entries (count == 0)", a);
            return REINA_E_INVALID;
        }
    memcpy(e->nrc, t->nr_contacts_by_age, sizeof(float) * A);
    memcpy(e->tcount, t->count, sizeof(int32_t) * A);
    memcpy(e->thr, t->threshold, sizeof(uint32_t) * A * REINA_MAX_ENTRIES);
    memcpy(e->meta, t->meta, sizeof(uint32_t) * A * REINA_MAX_ENTRIES);
    memcpy(e->mask_p, t->mask_p, sizeof(float) * A * 8);
    e->n_ranges = t->n_ranges;
    memcpy(e->range_min, t->range_min, sizeof(e->range_min));
    memcpy(e->range_max, t->range_max, sizeof(e->range_max));
    for (uint32_t a = 0; a < A; a++) rc_count_thresholds(e->nrc[a], e->cthr[a]);
    return 0;
}

/* ---------------------------------------------------------------- disease helpers */

/* Disease.get_symptom_severity (main.pyx:1042-1091), float32, variant 0 tables (quirk Q3);
 * both FATAL branches set DEATH_OUTSIDE_HOSPITAL (quirk Q2) */
static int severity_of(const Par *e, int age, float val, float vmod, int *pod_outside) {
    const reina_disease_t *d = &e->dis;
    float syc = d->p_symptomatic[age];
    *pod_outside = 0;
    if (val >= syc) return RV_ASYMPTOMATIC;
    syc *= vmod;
    float dohc = d->p_death_outside_hospital[age];
    if (dohc != 0.0f) {
        if (val < dohc * syc) {
            *pod_outside = 1;
            return RV_FATAL;
        }
        val = (val - dohc) / (1.0f - dohc);
    }
    float sc = d->p_severe_given_symptomatic[age];
    float cc = d->p_critical_given_severe[age];
    float fc = d->p_fatal_given_critical[age];
    if (val < fc * cc * sc * syc) {
        *pod_outside = 1;
        return RV_FATAL;
    }
    if (val < cc * sc * syc) return RV_CRITICAL;
    if (val < sc * syc) return RV_SEVERE;
    return RV_MILD;
}

static uint32_t clamp_days(Par *e, int d) {
    if (d < 0) d = 0;
    if (d > RH_MAX_DAYS) {
        set_problem(e, REINA_PROBLEM_DAYS_OVERFLOW);
        d = RH_MAX_DAYS;
    }
    return (uint32_t)d;
}

/* the source's half of person_infect (main.pyx:219-233): other_people_infected++, and the infectee appended to its list */
static void source_gains_infectee(Par *e, uint32_t s, int32_t infectee, uint32_t src_has_list) {
    int old = e->buf.cold[s].n_infected++;
    /* the source keeps an infectee list: its START-of-day word, carried in the candidate record
     * (person_expose_others runs before the source's own transition of the day, main.pyx:404-414) */
    if (!src_has_list) return;
    /* Person.infectees (main.pyx:128,231): the first REINA_INLINE_INFECTEES by rank in the source's inline block,
     * the others on its linked list -- threaded through the infectees' own records, or, when infectees may live on
     * another shard (exact attribution), through nodes of the pool */
    if (old >= 64) {
        set_problem(e, 1 /* TOO_MANY_INFECTEES */);
    } else if (old < REINA_INLINE_INFECTEES) {
        e->buf.infectees[(size_t)s * REINA_INLINE_INFECTEES + (uint32_t)old] = infectee;
    } else if (e->exact) {
        if ((uint32_t)CTL(e, REINA_L_POOL) >= e->cfg.pool_cap) {
            set_problem(e, REINA_PROBLEM_INFECTEE_POOL_OVERFLOW);
            return;
        }
        const uint32_t node = (uint32_t)CTL(e, REINA_L_POOL)++;
        e->buf.infectee_pool[2u * node] = (uint32_t)infectee;
        e->buf.infectee_pool[2u * node + 1u] = (uint32_t)e->buf.cold[s].first_infectee;
        e->buf.cold[s].first_infectee = (int32_t)node;
    } else {
        e->buf.cold[infectee].next_sibling = e->buf.cold[s].first_infectee;
        e->buf.cold[s].first_infectee = infectee;
    }
}

/* person_infect (main.pyx:209-235) + Population.infect (:1576-1582) */
static void install_infection(Par *e, uint32_t t, uint32_t day, uint32_t variant, int32_t src,
                              int fresh, uint32_t testing_mode, uint32_t src_has_list) {
    int age = age_of(e, t);
    uint32_t w = e->buf.hot[t];
    rp_u4 r = rp_philox(e->k0, e->k1, t, day, RP_P_INFECT, 0);
    float val = rp_uniform24(r.v[0]);
    float vmod = 1.0f;
    if ((w & RH_VACCINATED) && ((int)day - e->buf.cold[t].vacc_day > 14)) vmod = 0.1f;
    int pod = 0;
    int sev = severity_of(e, age, val, vmod, &pod);
    float g = rp_gamma_mu_cv(e->dis.mean_incubation_duration[0], 0.86f, e->k0, e->k1, t, day, RP_P_INFECT, 1);
    uint32_t dl = clamp_days(e, rp_round_to_int(g));
    uint32_t nw = RS_INCUBATION | ((uint32_t)sev << 3) | (variant << 8) | (pod ? RH_POD_OUTSIDE : 0) |
                  (w & (RH_VACCINATED | RH_DETECTED)) |   /* (was_detected outlives a re-infection: set_initial_state only) */
                  (testing_mode == RT_ALL_WITH_SYMPTOMS_CT ? RH_HASLIST : 0) | RH_ACTIVE |
                  /* (a FRESH agent of the initial condition sits out the scan of day 0 first) */
                  RH_DAYS_FIELD(dl, (fresh && day == RP_INIT_DAY) ? day + 1u : day) |
                  RH_INFECTED_ON((fresh && day == RP_INIT_DAY) ? day + 1u : day);
    e->buf.hot[t] = nw;
    if (src >= 0) {
        /* `src` is a global id when the population keeps them (exact attribution): the source's own shard counts the
         * infection and keeps the infectee list -- this one at once, another one when the day's feedback records arrive */
        e->buf.cold[t].infector = src;
        if (gid_local(e, src))
            source_gains_infectee(e, gid_index(e, src), gid_of(e, t), src_has_list);
        else
            xsend_push(e, rp_gid_shard((uint32_t)src), rp_xrec(gid_index(e, src), src_has_list << 2, (uint32_t)gid_of(e, t)));
    }
    CNT(e, REINA_C_SUSCEPTIBLE, age) -= 1;
    CNT(e, REINA_C_INFECTED, age) += 1;
    CNT(e, REINA_C_ALL_INFECTED, age) += 1;
    CNT(e, REINA_C_NEW_INFECTIONS, age) += 1;
    SC(e, REINA_S_INFECTED_BY_VARIANT + variant) += 1;
}

/* person_recover / person_die / person_become_removed (main.pyx:301-318,370-374) */
static uint32_t do_recover(Par *e, uint32_t w, int age) {
    CNT(e, REINA_C_INFECTED, age) -= 1;
    CNT(e, REINA_C_RECOVERED, age) += 1;
    return RH_SET_STATE(w, RS_RECOVERED) & ~RH_HASLIST;
}
static uint32_t do_die(Par *e, uint32_t w, int age) {
    CNT(e, REINA_C_INFECTED, age) -= 1;
    CNT(e, REINA_C_DEAD, age) += 1;
    if (w & RH_POD_OUTSIDE) CNT(e, REINA_C_NON_HOSPITAL_DEATHS, age) += 1;
    return RH_SET_STATE(w, RS_DEAD) & ~RH_HASLIST;
}

static void queue_append(Par *e, int which, uint32_t idx) {
    int l = which ? REINA_L_QUEUE1 : REINA_L_QUEUE0;
    uint32_t *q = which ? e->buf.queue1 : e->buf.queue0;
    if ((uint32_t)CTL(e, l) >= e->cfg.max_queue) {
        set_problem(e, REINA_PROBLEM_QUEUE_OVERFLOW);
        return;
    }
    q[CTL(e, l)++] = idx;
}

static void level1_append(Par *e, uint32_t idx) {
    if ((uint32_t)CTL(e, REINA_L_LEVEL1) >= e->cfg.max_queue) {
        set_problem(e, REINA_PROBLEM_QUEUE_OVERFLOW);
        return;
    }
    e->buf.level1[CTL(e, REINA_L_LEVEL1)++] = idx;
}

/* ---------------------------------------------------------------- imports (rounds) */
/* Population.infect_people / get_import_infection_person (main.pyx:1632-1665), parallel form.
 * Each import owns up to 10 tries (draws keyed by import number and try).  In a round every
 * unplaced import walks its remaining tries to the first one that hits a never-infected agent
 * and proposes it; a target proposed by several imports goes to the lowest import number, the
 * others go on with their next try in the next round (they would have met an infected agent). */
static int import_target(Par *e, const reina_day_t *dp, uint32_t j, uint32_t k, uint32_t *t_out) {
    const reina_disease_t *d = &e->dis;
    rp_u4 r = rp_philox(e->k0, e->k1, j, dp->day, RP_P_IMPORT, k);
    float p = rp_uniform24(r.v[0]);
    uint32_t c = d->n_import_classes - 1;
    for (uint32_t q = 0; q < d->n_import_classes; q++)
        if (p <= d->import_class_cum[q]) {
            c = q;
            break;
        }
    uint32_t start = (uint32_t)e->cfg.age_start[d->import_class_min_age[c]];
    uint32_t end = (uint32_t)e->cfg.age_start[d->import_class_max_age[c] + 1];
    if (end <= start) return 0;
    *t_out = start + r.v[1] % (end - start);
    return 1;
}

static void run_imports(Par *e, const reina_day_t *dp, int pre_init, uint32_t *import_base) {
    uint32_t total = 0;
    for (uint32_t b = 0; b < dp->n_import_batches; b++)
        if ((int)dp->import_batches[b].pre_init == pre_init) total += dp->import_batches[b].count;
    if (!total) return;
    uint32_t *variant = (uint32_t *)malloc(sizeof(uint32_t) * total);
    uint32_t *mode = (uint32_t *)malloc(sizeof(uint32_t) * total);   /* testing mode in force when the batch was imported */
    uint32_t *target = (uint32_t *)malloc(sizeof(uint32_t) * total);
    uint8_t *next_try = (uint8_t *)calloc(total, 1); /* 255 = placed */
    uint32_t n = 0;
    for (uint32_t b = 0; b < dp->n_import_batches; b++)
        if ((int)dp->import_batches[b].pre_init == pre_init)
            for (uint32_t k = 0; k < dp->import_batches[b].count; k++) {
                mode[n] = dp->import_batches[b].testing_mode;
                variant[n++] = dp->import_batches[b].variant;
            }
    /* Population.infect_people (main.pyx:1652-1665) as the reference runs it: one import after the other, each taking the
     * first of its <= 10 tries that hits a still susceptible agent.  (The HIP kernel reaches the same placement as a stable
     * matching -- targets prefer lower import numbers, imports earlier tries -- k_open.inc: pro_imports.) */
    for (uint32_t j = 0; j < total; j++)
        for (uint32_t k = 0; k < 10; k++) {
            uint32_t t;
            if (import_target(e, dp, *import_base + j, k, &t) && RH_STATE(e->buf.hot[t]) == RS_SUSCEPTIBLE) {
                install_infection(e, t, dp->day, variant[j], -1, 1, mode[j], 0);
                next_try[j] = 255;
                break;
            }
        }
    for (uint32_t j = 0; j < total; j++)
        if (next_try[j] != 255) SC(e, REINA_S_UNABLE_TO_IMPORT) += 1;
    *import_base += total;
    free(variant);
    free(mode);
    free(target);
    free(next_try);
}

/* ---------------------------------------------------------------- testing queue + tracing */
/* HealthcareSystem.queue_for_testing via contact tracing (main.pyx:474-488); the success roll is
 * keyed by (candidate, tracer) so that the SET of queued agents is order-free */
static int try_queue(Par *e, uint32_t cand, uint32_t tracer, const reina_day_t *dp) {
    uint32_t w = e->buf.hot[cand];
    if (RH_STATE(w) == RS_DEAD || (w & (RH_DETECTED | RH_QUEUED))) return 0;
    rp_u4 r = rp_philox(e->k0, e->k1, cand, dp->day, RP_P_TRACE, tracer);
    if (!rp_chance(dp->p_successful_tracing, r.v[0])) return 0;
    e->buf.hot[cand] = w | RH_QUEUED;
    return 1;
}

/* perform_contact_tracing (main.pyx:495-512) for one candidate of tracer `i`: a candidate of this shard is rolled for and
 * queued here; one that lives on another shard (exact attribution) becomes a request to its owner */
static void trace_candidate(Par *e, const reina_day_t *dp, int32_t g, uint32_t i, int level, int nxt) {
    if (g < 0) return;
    if (!gid_local(e, g)) {
        xsend_push(e, rp_gid_shard((uint32_t)g), rp_xrec(gid_index(e, g), 0, (uint32_t)gid_of(e, i)));
        return;
    }
    const uint32_t c = gid_index(e, g);
    if (try_queue(e, c, (uint32_t)gid_of(e, i), dp)) {
        queue_append(e, nxt, c);
        if (level == 0) level1_append(e, c);
    }
}

/* the infector and the infectees of agent i (level 0: a detected case; level 1: a contact queued at level 0) */
static void trace_from(Par *e, const reina_day_t *dp, uint32_t i, int level, int nxt) {
    trace_candidate(e, dp, e->buf.cold[i].infector, i, level, nxt);
    if (!(e->buf.hot[i] & RH_HASLIST)) return;
    for (int k = 0; k < REINA_INLINE_INFECTEES; k++)
        trace_candidate(e, dp, e->buf.infectees[(size_t)i * REINA_INLINE_INFECTEES + k], i, level, nxt);
    if (e->exact) {
        for (int32_t n = e->buf.cold[i].first_infectee; n >= 0; n = (int32_t)e->buf.infectee_pool[2u * (uint32_t)n + 1u])
            trace_candidate(e, dp, (int32_t)e->buf.infectee_pool[2u * (uint32_t)n], i, level, nxt);
    } else {
        for (int32_t c = e->buf.cold[i].first_infectee; c >= 0;) {
            const int32_t next = e->buf.cold[c].next_sibling;
            trace_candidate(e, dp, c, i, level, nxt);
            c = next;
        }
    }
}

/* HealthcareSystem.iterate (main.pyx:514-558), the test queue: detection and level-0 tracing of every detected case */
static void run_testing_level0(Par *e, const reina_day_t *dp) {
    int cur = dp->day & 1, nxt = cur ^ 1;
    uint32_t *q = cur ? e->buf.queue1 : e->buf.queue0;
    int lcur = cur ? REINA_L_QUEUE1 : REINA_L_QUEUE0;
    int n = CTL(e, lcur);
    SC(e, REINA_S_CT_CASES_PER_DAY) = n;
    /* Q1: every queued test is positive (quirk Q8) */
    for (int k = 0; k < n; k++) {
        uint32_t i = q[k];
        uint32_t w = e->buf.hot[i];
        if (w & RH_DETECTED) set_problem(e, 7 /* WRONG_STATE */);
        e->buf.hot[i] = (w & ~RH_QUEUED) | RH_DETECTED;
        int age = age_of(e, i);
        CNT(e, REINA_C_DETECTED, age) += 1;
        CNT(e, REINA_C_ALL_DETECTED, age) += 1;
    }
    CTL(e, REINA_L_LEVEL1) = 0;
    /* Q2: level 0 -- infector and infectees of every detected case */
    if (dp->testing_mode == RT_ALL_WITH_SYMPTOMS_CT)
        for (int k = 0; k < n; k++) trace_from(e, dp, q[k], 0, nxt);
    CTL(e, lcur) = 0;
}

/* Q3: level 1 -- the infector and infectees of everybody queued at level 0, no further recursion */
static void run_testing_level1(Par *e, const reina_day_t *dp) {
    if (dp->testing_mode != RT_ALL_WITH_SYMPTOMS_CT) return;
    const int nxt = (dp->day & 1) ^ 1;
    int n1 = CTL(e, REINA_L_LEVEL1);
    for (int k = 0; k < n1; k++) trace_from(e, dp, e->buf.level1[k], 1, nxt);
}

/* exact attribution: the tracing requests the other shards sent for candidates of this one */
static void run_trace_requests(Par *e, const reina_day_t *dp, int level) {
    const int nxt = (dp->day & 1) ^ 1;
    for (uint32_t sh = 0; sh < e->cfg.n_shards; sh++) {
        if (sh == e->cfg.shard_rank) continue;
        const uint64_t *seg = xseg(e, e->buf.xrecv, sh);
        const uint32_t n = xrecv_count(e, sh);
        for (uint32_t k = 0; k < n; k++) {
            const uint32_t c = rp_xrec_index(seg[1 + k]);
            if (try_queue(e, c, rp_xrec_gid(seg[1 + k]), dp)) {
                queue_append(e, nxt, c);
                if (level == 0) level1_append(e, c);
            }
        }
    }
    xsend_reset(e);
}

/* HealthcareSystem.vaccinate_people (main.pyx:560-583): oldest first, persistent cursor (agents
 * skipped once -- dead, detected or already vaccinated -- stay ineligible forever) */
static void run_vaccinations(Par *e, const reina_day_t *dp) {
    for (uint32_t k = 0; k < dp->n_vaccinations; k++) {
        const reina_vaccination_t *v = &dp->vaccinations[k];
        int32_t c = CTL(e, REINA_L_VACC_CURSOR + v->slot);
        if (c == INT_MIN) c = (int32_t)v->idx_end - 1;
        uint32_t nr = v->nr, done = 0;
        if (nr > v->idx_end - v->idx_start) nr = v->idx_end - v->idx_start;
        while (done < nr && c >= (int32_t)v->idx_start) {
            uint32_t i = (uint32_t)c;
            c--;
            uint32_t w = e->buf.hot[i];
            if (RH_STATE(w) == RS_DEAD || (w & (RH_VACCINATED | RH_DETECTED))) continue;
            e->buf.hot[i] = w | RH_VACCINATED;
            e->buf.cold[i].vacc_day = (int32_t)dp->day;
            CNT(e, REINA_C_VACCINATED, age_of(e, i)) += 1;
            done++;
        }
        CTL(e, REINA_L_VACC_CURSOR + v->slot) = c;
    }
}

/* ---------------------------------------------------------------- scan */
static void emit_event(Par *e, uint32_t i, uint32_t day, int type) {
    if ((uint32_t)CTL(e, REINA_L_HOSP) >= (e->cfg.max_hosp_events ? e->cfg.max_hosp_events : REINA_MAX_HOSP_EVENTS)) {
        set_problem(e, REINA_PROBLEM_HOSPITAL_OVERFLOW);
        return;
    }
    uint64_t prio = rp_priority20(e->k0, e->k1, i, day);
    e->buf.hosp_events[CTL(e, REINA_L_HOSP)++] = (prio << 34) | ((uint64_t)i << 2) | (uint64_t)type;
    if (type == EV_HOSPITALIZE) CTL(e, REINA_L_HOSP_ADMIT) += 1;
    if (type == EV_TO_ICU) CTL(e, REINA_L_ICU_ADMIT) += 1;
}

/* person_become_ill (main.pyx:284-291) + get_days_from_onset_to_removed / get_illness_days
 * (:989-1014) + HealthcareSystem.seek_testing (:595-615) */
static uint32_t onset_word(Par *e, uint32_t i, uint32_t w, uint32_t day) {
    int v = RH_VARIANT(w), sev = RH_SEV(w);
    float mu = sev == RV_FATAL ? e->dis.mean_duration_from_onset_to_death[v]
                               : e->dis.mean_duration_from_onset_to_recovery[v];
    float d = rp_gamma_mu_cv(mu, 0.45f, e->k0, e->k1, i, day, RP_P_ONSET, 1);
    e->buf.cold[i].onset_days = d;
    float f = d;
    if (sev >= RV_SEVERE) f *= e->dis.ratio_of_duration_before_hospitalisation[v];
    w = RH_SET_STATE(w, RS_ILLNESS);
    w = RH_SET_DAYS_LEFT(w, clamp_days(e, rp_round_to_int(f)), day);
    w = RH_SET_DOI0(w, day);
    return w;
}

static uint32_t become_ill(Par *e, uint32_t i, uint32_t w, const reina_day_t *dp) {
    int sev = RH_SEV(w);
    w = onset_word(e, i, w, dp->day);
    if (sev != RV_ASYMPTOMATIC && !(w & RH_DETECTED)) {
        int q = 0;
        if (dp->testing_mode == RT_ALL_WITH_SYMPTOMS || dp->testing_mode == RT_ALL_WITH_SYMPTOMS_CT) {
            q = 1;
        } else if (dp->testing_mode == RT_ONLY_SEVERE_SYMPTOMS) {
            if (sev >= RV_SEVERE)
                q = 1;
            else
                q = rp_chance(dp->p_detected_anyway, rp_philox(e->k0, e->k1, i, dp->day, RP_P_ONSET, 0).v[3]);
        }
        if (q && !(w & RH_QUEUED)) {
            w |= RH_QUEUED;
            queue_append(e, (dp->day & 1) ^ 1, i);
        }
    }
    return w;
}

/* Context._process_person + person_advance (main.pyx:1968-1979, 395-438) for every agent */
static void run_scan(Par *e, const reina_day_t *dp) {
    uint32_t N = e->cfg.n_agents;
    const reina_disease_t *d = &e->dis;
    for (uint32_t i = 0; i < N; i++) {
        uint32_t w = e->buf.hot[i];
        uint32_t st = RH_STATE(w);
        if (st == RS_SUSCEPTIBLE) continue;
        if (st >= RS_RECOVERED) {
            if (!(w & RH_INCLUDED)) {
                SC(e, REINA_S_TOTAL_INFECTORS) += 1;
                SC(e, REINA_S_TOTAL_INFECTIONS) += e->buf.cold[i].n_infected;
                e->buf.hot[i] = (w | RH_INCLUDED) & ~RH_ACTIVE;
            }
            continue;
        }
        if (RH_INFECTED_TODAY(w, dp->day)) {   /* infected earlier today (an import): waits, main.pyx:402 */
            continue;
        }
        int age = age_of(e, i);
        int v = RH_VARIANT(w), sev = RH_SEV(w);
        uint32_t dl = RH_DAYS_LEFT(w, dp->day);   /* absolute days in the word: waiting leaves it unchanged */
        if (st == RS_INCUBATION || st == RS_ILLNESS) {
            /* person_expose_others -> get_exposed_people -> get_contacts (main.pyx:247-281,936-955,
             * 1308-1320,1539-1573): only the COUNT is drawn here, contacts are realised later */
            int nr = 0;
            if (!(w & RH_DETECTED)) {
                int dayrel = st == RS_INCUBATION ? -(int)dl : (int)RH_DOI(w, dp->day);
                float inf = (dayrel >= -10 && dayrel <= 10) ? d->infectiousness_over_time[v][dayrel + 10] : 0.0f;
                if (inf != 0.0f) {
                    /* get_nr_contacts (main.pyx:1308-1320) by inversion of the day's draw through the count thresholds
                     * of the agent's age; an agent with symptoms draws from the (factor 0.5, limit 5) class */
                    nr = rc_count_from_draw(e->cthr[age], st == RS_ILLNESS && sev != RV_ASYMPTOMATIC,
                                            rp_count_draw(e->k0, e->k1, i, dp->day));
                    if (nr > 0) {
                        float src_inf = inf;
                        if (sev == RV_ASYMPTOMATIC) src_inf *= d->p_asymptomatic_infection[v];
                        if ((uint32_t)CTL(e, REINA_L_WORK) >= e->cfg.max_work_items) {
                            set_problem(e, REINA_PROBLEM_WORK_OVERFLOW);
                        } else {
                            uint32_t *wi = e->buf.work_items + 4u * (uint32_t)CTL(e, REINA_L_WORK)++;
                            wi[0] = i;
                            wi[1] = (uint32_t)nr | ((uint32_t)v << 8) | ((uint32_t)age << 16);
                            wi[2] = rp_f2u(src_inf);
                            wi[3] = (w & RH_HASLIST) ? 1u : 0u;
                        }
                    }
                }
            }
            SC(e, REINA_S_EXPOSED_PER_DAY) += nr;
            if (st == RS_INCUBATION) {
                if (dl > 0) dl--;
                if (dl == 0) w = become_ill(e, i, w, dp);
            } else {
                if (dl > 0) dl--;
                if (dl == 0) {
                    if (sev == RV_FATAL && (w & RH_POD_OUTSIDE))
                        w = do_die(e, w, age);
                    else if (sev >= RV_SEVERE)
                        emit_event(e, i, dp->day, EV_HOSPITALIZE);
                    else
                        w = do_recover(e, w, age);
                }
            }
        } else if (st == RS_HOSPITALIZED) {
            if (dl > 0) dl--;
            if (dl == 0) emit_event(e, i, dp->day, sev >= RV_CRITICAL ? EV_TO_ICU : EV_RELEASE_WARD);
        } else { /* IN_ICU */
            if (dl > 0) dl--;
            if (dl == 0) emit_event(e, i, dp->day, EV_RELEASE_ICU);
        }
        e->buf.hot[i] = w;
    }
}

/* ---------------------------------------------------------------- hospital events */
static int cmp_u64(const void *a, const void *b) {
    uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b;
    return x < y ? -1 : (x > y ? 1 : 0);
}

/* Disease.dies_in_hospital (main.pyx:957-974) */
static int dies_in_hospital(Par *e, uint32_t i, uint32_t day, int sev, int v, int care) {
    if (sev == RV_FATAL) return 1;
    float p = 0.0f;
    if (sev == RV_CRITICAL) {
        if (care) return 0;
        p = e->dis.p_icu_death_no_beds[v];
    } else if (sev == RV_SEVERE) {
        if (care) return 0;
        p = e->dis.p_hospital_death_no_beds[v];
    }
    return rp_chance(p, rp_philox(e->k0, e->k1, i, day, RP_P_HOSPITAL, 0).v[0]);
}

/* person_hospitalize / transfer_to_icu / release_from_hospital (main.pyx:321-367) +
 * HealthcareSystem bed accounting (:617-651), in priority order when capacity can bind */
static void run_hospital_events(Par *e, const reina_day_t *dp);

static void run_hospital(Par *e, const reina_day_t *dp) {
    run_hospital_events(e, dp);
}

/* one event applied to its agent; *b, *c: free beds / ICU units, moved as the reference's counters move */
static void apply_hospital_event(Par *e, const reina_day_t *dp, uint64_t ev, int *b, int *c) {
    const reina_disease_t *d = &e->dis;
    int type = (int)(ev & 3);
    uint32_t i = (uint32_t)((ev >> 2) & 0xFFFFFFFFu);
    uint32_t w = e->buf.hot[i];
    int age = age_of(e, i), v = RH_VARIANT(w), sev = RH_SEV(w);
    float od = e->buf.cold[i].onset_days;
    if (type == EV_HOSPITALIZE) {
        if (!(w & RH_DETECTED)) {
            w |= RH_DETECTED;
            CNT(e, REINA_C_DETECTED, age) += 1;
            CNT(e, REINA_C_ALL_DETECTED, age) += 1;
        }
        if (*b == 0) {
            w = dies_in_hospital(e, i, dp->day, sev, v, 0) ? do_die(e, w, age) : do_recover(e, w, age);
        } else {
            (*b)--;
            const float f = rp_ward_stay(sev, od, d->ratio_of_duration_before_hospitalisation[v], d->ratio_of_duration_in_ward[v]);
            w = RH_SET_DAYS_LEFT(RH_SET_STATE(w, RS_HOSPITALIZED), clamp_days(e, rp_round_to_int(f)), dp->day);
            CNT(e, REINA_C_HOSPITALIZED, age) += 1;
            CNT(e, REINA_C_IN_WARD, age) += 1;
        }
    } else if (type == EV_TO_ICU) {
        (*b)++;
        int ok = *c > 0;
        if (ok) (*c)--;
        if (!ok && dies_in_hospital(e, i, dp->day, sev, v, 0)) {
            CNT(e, REINA_C_IN_WARD, age) -= 1;
            CNT(e, REINA_C_HOSPITALIZED, age) -= 1;
            w = do_die(e, w, age);
        } else {
            const float f = rp_icu_stay(sev, od, d->ratio_of_duration_before_hospitalisation[v], d->ratio_of_duration_in_ward[v]);
            w = RH_SET_DAYS_LEFT(RH_SET_STATE(w, RS_IN_ICU), clamp_days(e, rp_round_to_int(f)), dp->day);
            CNT(e, REINA_C_IN_WARD, age) -= 1;
            CNT(e, REINA_C_IN_ICU, age) += 1;
            CNT(e, REINA_C_CUM_ICU, age) += 1;
        }
    } else if (type == EV_RELEASE_WARD) {
        CNT(e, REINA_C_IN_WARD, age) -= 1;
        CNT(e, REINA_C_HOSPITALIZED, age) -= 1;
        (*b)++;
        w = dies_in_hospital(e, i, dp->day, sev, v, 1) ? do_die(e, w, age) : do_recover(e, w, age);
    } else {
        CNT(e, REINA_C_IN_ICU, age) -= 1;
        CNT(e, REINA_C_HOSPITALIZED, age) -= 1;
        (*c)++;
        w = dies_in_hospital(e, i, dp->day, sev, v, 1) ? do_die(e, w, age) : do_recover(e, w, age);
    }
    e->buf.hot[i] = w;
}

/* the map of one event on the free beds / free ICU units (reina_prims.h: rp_sat_t) */
static rp_sat_t bed_map(int type) {
    rp_sat_t f = rp_sat_id();
    if (type == EV_HOSPITALIZE) { f.a = -1; f.m = 0; }
    else if (type == EV_TO_ICU || type == EV_RELEASE_WARD) f.a = 1;
    return f;
}
static rp_sat_t icu_map(int type) {
    rp_sat_t f = rp_sat_id();
    if (type == EV_TO_ICU) { f.a = -1; f.m = 0; }
    else if (type == EV_RELEASE_ICU) f.a = 1;
    return f;
}
static uint32_t event_bucket(const Par *e, uint64_t ev) { return (uint32_t)(ev >> 34) >> (20u - e->hosp_range_bits); }
static uint64_t *exchange_maps(Par *e, uint32_t shard) {
    return (uint64_t *)(e->buf.pressure + REINA_PRESSURE_WORDS) + (size_t)shard * e->hosp_ranges;
}

/* a SHARDED population, first half of the day: the day's events sorted, every priority bucket's composed map into this
 * shard's segment of the exchange block (include/reina_hip.h: REINA_EXCHANGE_WORDS) */
static void publish_hospital_maps(Par *e) {
    int M = CTL(e, REINA_L_HOSP);
    qsort(e->buf.hosp_events, (size_t)M, sizeof(uint64_t), cmp_u64);
    uint64_t *seg = exchange_maps(e, e->cfg.shard_rank);
    for (int k = 0; k < M;) {
        const uint32_t bk = event_bucket(e, e->buf.hosp_events[k]);
        rp_sat_t fb = rp_sat_id(), fc = rp_sat_id();
        for (; k < M && event_bucket(e, e->buf.hosp_events[k]) == bk; k++) {
            const int type = (int)(e->buf.hosp_events[k] & 3);
            fb = rp_sat_then(fb, bed_map(type));
            fc = rp_sat_then(fc, icu_map(type));
        }
        seg[bk] = rp_sat_pack(fb, fc);
    }
}

static void run_hospital_events(Par *e, const reina_day_t *dp) {
    int M = CTL(e, REINA_L_HOSP);
    if (e->cfg.n_shards > 1) {
        /* ONE pool of beds / ICU units for all shards (the reference: one counter, main.pyx:617-651).  The all-reduce has
         * brought every shard's free counts at day open, its demand, and the map of every priority bucket of its events.
         * Global order of the day's events: (priority bucket, shard, priority, agent) -- this shard walks its own events
         * and lets the other shards' buckets act on the pool through their maps. */
        int64_t fb = 0, fc = 0, db = 0, dc = 0;
        for (uint32_t sh = 0; sh < e->cfg.n_shards; sh++) {
            fb += e->buf.pressure[REINA_PRESSURE_FREE_BEDS(sh)];
            fc += e->buf.pressure[REINA_PRESSURE_FREE_ICU(sh)];
            db += e->buf.pressure[REINA_PRESSURE_DEMAND_BEDS(sh)];
            dc += e->buf.pressure[REINA_PRESSURE_DEMAND_ICU(sh)];
        }
        int b = (int)fb, c = (int)fc;
        int own_b = 0, own_c = 0;   /* the pool's net change by this shard's events */
        if (fb >= db && fc >= dc) {
            /* nothing can run out anywhere: every request granted */
            for (int k = 0; k < M; k++) {
                int b0 = b, c0 = c;
                apply_hospital_event(e, dp, e->buf.hosp_events[k], &b, &c);
                own_b += b - b0;
                own_c += c - c0;
            }
        } else {
            int k = 0;
            for (uint32_t bk = 0; bk < e->hosp_ranges; bk++)
                for (uint32_t sh = 0; sh < e->cfg.n_shards; sh++) {
                    if (sh != e->cfg.shard_rank) {
                        rp_sat_t gb, gc;
                        rp_sat_unpack(exchange_maps(e, sh)[bk], &gb, &gc);
                        b = rp_sat_apply(gb, b);
                        c = rp_sat_apply(gc, c);
                        continue;
                    }
                    for (; k < M && event_bucket(e, e->buf.hosp_events[k]) == bk; k++) {
                        int b0 = b, c0 = c;
                        apply_hospital_event(e, dp, e->buf.hosp_events[k], &b, &c);
                        own_b += b - b0;
                        own_c += c - c0;
                    }
                }
        }
        SC(e, REINA_S_AVAILABLE_BEDS) += own_b;
        SC(e, REINA_S_AVAILABLE_ICU) += own_c;
        return;
    }
    if (!M) return;
    int b = SC(e, REINA_S_AVAILABLE_BEDS), c = SC(e, REINA_S_AVAILABLE_ICU);
    if (!(b >= CTL(e, REINA_L_HOSP_ADMIT) && c >= CTL(e, REINA_L_ICU_ADMIT)))
        qsort(e->buf.hosp_events, (size_t)M, sizeof(uint64_t), cmp_u64);
    for (int k = 0; k < M; k++) apply_hospital_event(e, dp, e->buf.hosp_events[k], &b, &c);
    SC(e, REINA_S_AVAILABLE_BEDS) = b;
    SC(e, REINA_S_AVAILABLE_ICU) = c;
}

/* ---------------------------------------------------------------- initial population condition */
/* Population.set_initial_state (main.pyx:1452-1516), parallel form (include/reina_hip.h:
 * reina_set_initial_state).  Slot j draws ONE uniform agent, with replacement like get_random_person
 * (main.pyx:1518-1520) -- an agent drawn by several slots is visited by them in slot order and ends as the last one
 * leaves it, while every visit moves the counters (person_infect on an infected, recovered or dead person is
 * what the reference does; in a 20 000-agent population with 430 initial agents that is 4.6 agents per run, and a
 * later `recovered` slot takes out an earlier ill one: 1.4 % of the infectious seed).  Capacity: ICU-fated slots come
 * first and hand their bed back when they move to ICU (hc.to_icu, main.pyx:641-646), so the r-th ICU slot gets a unit
 * iff r < units and the r-th ward slot a bed iff r < beds.  Not reproduced: the reference's transfer_to_icu of an
 * agent who was just refused a bed (only reachable with zero beds). */
static int initial_target(Par *e, uint32_t slot, uint32_t k, uint32_t *t_out) {
    rp_u4 r = rp_philox(e->k0, e->k1, slot, RP_INIT_DAY, RP_P_INITIAL, k);
    *t_out = r.v[0] % e->cfg.n_agents;
    return 1;
}

int par_set_initial_state(Par *e, const reina_initial_state_t *ic, void *stream) {
    (void)stream;
    if (!e->bound) return REINA_E_NOT_BOUND;
    if (e->cfg.n_shards <= 1 && ic->in_icu > 0 && SC(e, REINA_S_BEDS) == 0 &&
        (uint64_t)ic->were_incubating > (uint64_t)ic->incubating + ic->recovered_without_illness + ic->ill + ic->dead)
        return REINA_E_INVALID;   /* the reference refuses a walk that REACHES an ICU slot when the hospital has no beds
                                     (main.pyx:1495 -> :350 -> :1603); a walk cut short before them constructs (:1456-1463) */
    const uint32_t M = ic->were_incubating;
    const uint32_t i_inc = ic->incubating, i_rec = i_inc + ic->recovered_without_illness, i_ill = i_rec + ic->ill,
                   i_dead = i_ill + ic->dead, i_icu = i_dead + ic->in_icu, i_ward = i_icu + ic->in_ward;
    const reina_disease_t *d = &e->dis;
    int b = SC(e, REINA_S_AVAILABLE_BEDS), c = SC(e, REINA_S_AVAILABLE_ICU);
    const int beds0 = b, icu0 = c;
    {
    {
        for (uint32_t j = 0; j < M; j++) {
            uint32_t t;
            initial_target(e, j, 0, &t);
            install_infection(e, t, RP_INIT_DAY, 0, -1, j < i_inc, RT_NO_TESTING, 0);
            if (j < i_inc) continue;
            uint32_t w = e->buf.hot[t];
            const int age = age_of(e, t);
            if (j < i_rec) {
                e->buf.hot[t] = do_recover(e, w, age);
                continue;
            }
            w = onset_word(e, t, w, RP_INIT_DAY);
            const int v = RH_VARIANT(w), sev = RH_SEV(w);
            const float od = e->buf.cold[t].onset_days;
            if (j < i_ill) {
            } else if (j < i_dead) {
                w = do_die(e, w, age);
            } else if (j < i_ward) {
                const int to_icu = j < i_icu;
                if (!(w & RH_DETECTED)) {   /* person_hospitalize detects first (main.pyx:322-325), once per person */
                    w |= RH_DETECTED;
                    CNT(e, REINA_C_DETECTED, age) += 1;
                    CNT(e, REINA_C_ALL_DETECTED, age) += 1;
                }
                /* (an ICU-bound agent hands its bed back at once: it gets one iff the hospital -- of the whole population --
                 * has any, which the caller has checked: the reference does not construct otherwise) */
                const int bed = to_icu ? 1 : (int)(j - i_icu) < beds0;
                if (!bed) {
                    w = dies_in_hospital(e, t, RP_INIT_DAY, sev, v, 0) ? do_die(e, w, age) : do_recover(e, w, age);
                } else if (!to_icu) {
                    b--;
                    const float f = rp_ward_stay(sev, od, d->ratio_of_duration_before_hospitalisation[v], d->ratio_of_duration_in_ward[v]);
                    w = RH_SET_DAYS_LEFT(RH_SET_STATE(w, RS_HOSPITALIZED), clamp_days(e, rp_round_to_int(f)), RP_INIT_DAY);
                    CNT(e, REINA_C_HOSPITALIZED, age) += 1;
                    CNT(e, REINA_C_IN_WARD, age) += 1;
                } else {
                    const int unit = (int)(j - i_dead) < icu0;
                    if (unit) c--;
                    if (!unit && dies_in_hospital(e, t, RP_INIT_DAY, sev, v, 0)) {
                        w = do_die(e, w, age);   /* hospitalised and released at once: no net ward count */
                    } else {
                        const float f = rp_icu_stay(sev, od, d->ratio_of_duration_before_hospitalisation[v], d->ratio_of_duration_in_ward[v]);
                        w = RH_SET_DAYS_LEFT(RH_SET_STATE(w, RS_IN_ICU), clamp_days(e, rp_round_to_int(f)), RP_INIT_DAY);
                        CNT(e, REINA_C_HOSPITALIZED, age) += 1;
                        CNT(e, REINA_C_IN_ICU, age) += 1;
                        CNT(e, REINA_C_CUM_ICU, age) += 1;
                    }
                }
            } else {
                w = do_recover(e, w, age);
            }
            e->buf.hot[t] = w;
        }
    }
    }
    SC(e, REINA_S_AVAILABLE_BEDS) = b;
    SC(e, REINA_S_AVAILABLE_ICU) = c;
    /* main.pyx:1503-1516 */
    for (uint32_t a = 0; a < 100 && a < e->cfg.nr_ages; a++) CNT(e, REINA_C_ALL_DETECTED, a) = 0;
    const uint32_t stride = ic->confirmed_stride ? ic->confirmed_stride : 1;
    for (uint32_t i = ic->confirmed_first; i < ic->confirmed_cases; i += stride)
        if (i % 100 < e->cfg.nr_ages) CNT(e, REINA_C_ALL_DETECTED, i % 100) += 1;
    return 0;
}

/* ---------------------------------------------------------------- contacts + install */
/* get_one_contact / get_person_from_age_range / person_expose / did_infect
 * (main.pyx:1290-1304,1525-1535,238-244,908-934) for every sampled contact */
static void run_contacts(Par *e, const reina_day_t *dp) {
    const reina_disease_t *d = &e->dis;
    int W = CTL(e, REINA_L_WORK);
    for (int k = 0; k < W; k++) {
        const uint32_t *wi = e->buf.work_items + 4u * (uint32_t)k;
        uint32_t src = wi[0];
        int nr = (int)(wi[1] & 0xFF), v = (int)((wi[1] >> 8) & 0xFF), row = (int)(wi[1] >> 16);
        float src_inf = rp_u2f(wi[2]);
        uint32_t prio = rp_priority20(e->k0, e->k1, src, dp->day);
        uint64_t key = rp_order_key(dp->day, prio, (uint32_t)gid_of(e, src));
        for (int c = 0; c < nr; c++) {
            /* Philox2x32: half 0 = (place / age-range draw, transmission draw), half 1 = (shard + target draw, mask draw) */
            const uint32_t ckey = rp_contact_key(e->k0, e->k1);
            const rp_u2 q0 = rp_philox2(ckey, src, rp_contact_ctr(dp->day, (uint32_t)c, 0));
            const rp_u2 q1 = rp_philox2(ckey, src, rp_contact_ctr(dp->day, (uint32_t)c, 1));
            rp_u4 r;   /* (the names of the four draws as the formulation uses them) */
            r.v[0] = q0.v[0]; r.v[2] = q0.v[1]; r.v[1] = q1.v[0]; r.v[3] = q1.v[1];
            int cnt = e->tcount[row];
            int ent = cnt - 1;
            for (int j = 0; j < cnt; j++)
                if (r.v[0] < e->thr[row][j]) {
                    ent = j;
                    break;
                }
            uint32_t m = e->meta[row][ent];
            int place = (int)(m & 0xFF), cmin = (int)((m >> 8) & 0xFF), cmax = (int)((m >> 16) & 0xFF);
            uint32_t range_id = m >> 24;
            uint32_t start = (uint32_t)e->cfg.age_start[cmin], end = (uint32_t)e->cfg.age_start[cmax + 1];
            SC(e, REINA_S_DAILY_CONTACTS + place) += 1;
            CTL(e, REINA_L_CONTACTS) += 1;
            /* the contact is a uniform member of the age range over the WHOLE population: uniform
             * shard, then uniform agent of that shard (every shard holds 1/G of every age) */
            const uint32_t G = e->cfg.n_shards;
            uint32_t dest = r.v[1] % G;
            if (dest != e->cfg.shard_rank && e->exact) {
                /* exact attribution: the source completes did_infect (main.pyx:908-934) itself -- age ranges are global
                 * knowledge, so it draws the target on the other shard and knows its age -- and sends (target, source id,
                 * variant, list flag); all the destination adds is person_expose's test (main.pyx:239) and the claim */
                const int32_t *das = e->shard_age_start[dest];
                const uint32_t ds = (uint32_t)das[cmin], de = (uint32_t)das[cmax + 1];
                if (de <= ds) continue;
                if (!rp_chance(src_inf * e->psus_max[v] * d->infectiousness_multiplier[v], r.v[2])) continue;   /* (as below) */
                const uint32_t t = ds + (r.v[1] / G) % (de - ds);
                int age_t = cmin;
                while (age_t < cmax && (uint32_t)das[age_t + 1] <= t) age_t++;
                if (!rp_chance(src_inf * d->p_susceptibility[v][age_t] * d->infectiousness_multiplier[v], r.v[2])) continue;
                const float mp = e->mask_p[row][place];
                if (mp != 0.0f) {
                    float a = mp * d->p_mask_protects_others[v];
                    float b = mp * d->p_mask_protects_wearer[v];
                    float pm = a + b - a * b;
                    if (rp_chance(pm, r.v[3])) continue;
                }
                xsend_push(e, dest, rp_xrec(t, (uint32_t)v | (wi[3] << 2), (uint32_t)gid_of(e, src)));
                continue;
            }
            if (dest != e->cfg.shard_rank) {
                /* source-side part of did_infect: everything that does not depend on the target;
                 * the target's susceptibility is applied by the destination as p_sus / psus_max */
                float q = src_inf * e->psus_max[v] * d->infectiousness_multiplier[v];
                if (!rp_chance(q, r.v[2])) continue;
                float mp = e->mask_p[row][place];
                if (mp != 0.0f) {
                    float a = mp * d->p_mask_protects_others[v];
                    float b = mp * d->p_mask_protects_wearer[v];
                    float pm = a + b - a * b;
                    if (rp_chance(pm, r.v[3])) continue;
                }
                e->buf.pressure[(dest * REINA_MAX_RANGES + range_id) * REINA_MAX_VARIANTS + (uint32_t)v] += 1;
                /* mirror table: keep the smallest (tie-break, src) per slot, tagged with today */
                {
                    rp_u4 hm = rp_philox(e->k0, e->k1, src, dp->day, RP_P_MIRROR, (uint32_t)c);
                    uint32_t S = e->cfg.mirror_slots, cell = range_id * REINA_MAX_VARIANTS + (uint32_t)v;
                    uint32_t eff = e->buf.mirror_meta[cell];   /* slots of this cell in use today */
                    uint64_t *slot = e->buf.mirror + (size_t)cell * S + (hm.v[0] & (eff - 1));
                    uint64_t ent = rp_order_key(dp->day, hm.v[1] >> 12, src);
                    if (ent < *slot) *slot = ent;
                    e->buf.mirror_meta[REINA_MIRROR_CELLS + cell] = dp->day + 1;
                }
                continue;
            }
            if (end <= start) continue;
            /* a draw that is not below the source's LARGEST possible transmission probability cannot infect
             * whoever is met: skip the look at the target (same outcome, far fewer random reads on the host) */
            if (!rp_chance(src_inf * e->psus_max[v] * d->infectiousness_multiplier[v], r.v[2])) continue;
            uint32_t t = start + (r.v[1] / G) % (end - start);
            if (RH_STATE(e->buf.hot[t]) != RS_SUSCEPTIBLE) continue;   /* person_expose, main.pyx:239 */
            int age_t = age_of(e, t);
            float p = src_inf * d->p_susceptibility[v][age_t] * d->infectiousness_multiplier[v];
            if (!rp_chance(p, r.v[2])) continue;
            float mp = e->mask_p[row][place];
            if (mp != 0.0f) {
                float a = mp * d->p_mask_protects_others[v];
                float b = mp * d->p_mask_protects_wearer[v];
                float pm = a + b - a * b;
                if (rp_chance(pm, r.v[3])) continue;
            }
            if (key < e->buf.cold[t].claim) e->buf.cold[t].claim = key;
            if ((uint32_t)CTL(e, REINA_L_CAND) >= e->cfg.max_candidates) {
                set_problem(e, REINA_PROBLEM_CANDIDATE_OVERFLOW);
                continue;
            }
            uint32_t *cd = e->buf.candidates + 4u * (uint32_t)CTL(e, REINA_L_CAND)++;
            cd[0] = t;
            cd[1] = (uint32_t)gid_of(e, src);
            cd[2] = (uint32_t)v | (wi[3] << 8);
            cd[3] = prio;
        }
    }
}

/* exact attribution: the contact records the other shards sent.  A record stands for a contact that passed did_infect's
 * whole test at its source; here it meets person_expose's test (only a never-infected agent can be infected,
 * main.pyx:239) and competes for the target like a local contact, under its source's own key */
static void run_remote_exact(Par *e, const reina_day_t *dp) {
    for (uint32_t sh = 0; sh < e->cfg.n_shards; sh++) {
        if (sh == e->cfg.shard_rank) continue;
        const uint64_t *seg = xseg(e, e->buf.xrecv, sh);
        const uint32_t n = xrecv_count(e, sh);
        for (uint32_t k = 0; k < n; k++) {
            const uint32_t t = rp_xrec_index(seg[1 + k]), fl = rp_xrec_flags(seg[1 + k]), src = rp_xrec_gid(seg[1 + k]);
            if (RH_STATE(e->buf.hot[t]) != RS_SUSCEPTIBLE) continue;
            const uint32_t prio = rp_priority20(e->shard_k0[sh], e->shard_k1[sh], src & RP_GID_INDEX_MASK, dp->day);
            const uint64_t key = rp_order_key(dp->day, prio, src);
            if (key < e->buf.cold[t].claim) e->buf.cold[t].claim = key;
            if ((uint32_t)CTL(e, REINA_L_CAND) >= e->cfg.max_candidates) {
                set_problem(e, REINA_PROBLEM_CANDIDATE_OVERFLOW);
                continue;
            }
            uint32_t *cd = e->buf.candidates + 4u * (uint32_t)CTL(e, REINA_L_CAND)++;
            cd[0] = t;
            cd[1] = src;
            cd[2] = (fl & 3u) | ((fl >> 2) << 8);
            cd[3] = prio;
        }
    }
    xsend_reset(e);
}

/* exact attribution: the feedback records of the day's cross-shard infections -- the sources that live here take their
 * infectees (person_infect's source half, main.pyx:219-233), so that counts and lists are true before the next morning */
static void run_feedback(Par *e) {
    for (uint32_t sh = 0; sh < e->cfg.n_shards; sh++) {
        if (sh == e->cfg.shard_rank) continue;
        const uint64_t *seg = xseg(e, e->buf.xrecv, sh);
        const uint32_t n = xrecv_count(e, sh);
        for (uint32_t k = 0; k < n; k++)
            source_gains_infectee(e, rp_xrec_index(seg[1 + k]), (int32_t)rp_xrec_gid(seg[1 + k]), rp_xrec_flags(seg[1 + k]) >> 2);
    }
    xsend_reset(e);
}

/* cross-shard pressure aimed at this shard (summed over all shards by the caller): attempt k of
 * cell (range, variant) picks a uniform local agent of the range and passes the target-side part
 * of did_infect, p_sus(age) / psus_max; it then competes for the target like a local contact */
static void run_remote(Par *e, const reina_day_t *dp) {
    const reina_disease_t *d = &e->dis;
    if (e->cfg.n_shards <= 1) return;
    if (e->exact) {
        run_remote_exact(e, dp);
        return;
    }
    uint32_t idx = 0;
    for (uint32_t rg = 0; rg < e->n_ranges; rg++)
        for (uint32_t v = 0; v < e->cfg.nr_variants; v++) {
            int n = e->buf.pressure[(e->cfg.shard_rank * REINA_MAX_RANGES + rg) * REINA_MAX_VARIANTS + v];
            uint32_t start = (uint32_t)e->cfg.age_start[e->range_min[rg]];
            uint32_t end = (uint32_t)e->cfg.age_start[e->range_max[rg] + 1];
            for (int k = 0; k < n; k++, idx++) {
                if (end <= start) continue;
                rp_u4 r = rp_philox(e->k0, e->k1, (uint32_t)k, dp->day, RP_P_REMOTE, rg | (v << 8));
                uint32_t t = start + r.v[0] % (end - start);
                if (RH_STATE(e->buf.hot[t]) != RS_SUSCEPTIBLE) continue;   /* person_expose, main.pyx:239 */
                int age_t = age_of(e, t);
                float p = d->p_susceptibility[v][age_t] / e->psus_max[v];
                if (!rp_chance(p, r.v[1])) continue;
                uint32_t prio = r.v[2] >> 12;
                /* mirror attribution: first slot at/after a hashed start holding an entry of today;
                 * own cell first, then the other ranges of the variant, then the other variants */
                uint32_t src = RP_REMOTE_SRC | idx;
                {
                    uint32_t S = e->cfg.mirror_slots;
                    int found = 0;
                    for (uint32_t dv = 0; dv < e->cfg.nr_variants && !found; dv++)
                        for (uint32_t dr = 0; dr < e->n_ranges && !found; dr++) {
                            uint32_t cell = ((rg + dr) % e->n_ranges) * REINA_MAX_VARIANTS + (v + dv) % e->cfg.nr_variants;
                            if (e->buf.mirror_meta[REINA_MIRROR_CELLS + cell] != dp->day + 1) continue;   /* nothing today */
                            const uint32_t eff = e->buf.mirror_meta[cell];
                            const uint32_t probes = eff < RP_MIRROR_PROBES ? eff : RP_MIRROR_PROBES;
                            const uint64_t *tab = e->buf.mirror + (size_t)cell * S;
                            for (uint32_t j = 0; j < probes; j++) {
                                uint64_t ent = tab[(r.v[3] + j) & (eff - 1)];
                                /* (not removed by today's scan: k_remote.inc) */
                                if ((ent >> 52) == ((4095u - dp->day) & 0xFFFu) &&
                                    (((uint32_t)ent & RP_REMOTE_SRC) || RH_STATE(e->buf.hot[(uint32_t)ent]) < RS_RECOVERED)) {
                                    src = (uint32_t)ent;
                                    found = 1;
                                    break;
                                }
                            }
                        }
                    /* nobody on this shard aimed at another shard today (a small outbreak: a handful of infectious agents
                     * per shard): the most recent entry of the last RP_MIRROR_STALE_DAYS days stands in, same order of cells --
                     * without it about one infection in ten of such an outbreak had no infector link and contact tracing
                     * could not reach it (4 shards, 31 000 agents, tracing at 92 %: DESIGN section 6) */
                    for (uint32_t dv = 0; dv < e->cfg.nr_variants && !found; dv++)
                        for (uint32_t dr = 0; dr < e->n_ranges && !found; dr++) {
                            uint32_t cell = ((rg + dr) % e->n_ranges) * REINA_MAX_VARIANTS + (v + dv) % e->cfg.nr_variants;
                            const uint32_t last = e->buf.mirror_meta[REINA_MIRROR_CELLS + cell];   /* day + 1 of the last insertion */
                            if (last == 0 || dp->day + 1u - last > RP_MIRROR_STALE_DAYS) continue;
                            const uint32_t eff = e->buf.mirror_meta[cell];
                            const uint32_t probes = eff < RP_MIRROR_PROBES ? eff : RP_MIRROR_PROBES;
                            const uint64_t *tab = e->buf.mirror + (size_t)cell * S;
                            uint64_t best = ~0ull;
                            for (uint32_t j = 0; j < probes; j++) {
                                uint64_t ent = tab[(r.v[3] + j) & (eff - 1)];
                                if (ent < best) best = ent;   /* (smaller key = later day) */
                            }
                            /* ... if it has not been removed since (k_remote.inc: the R statistics of an agent first seen
                             * removed today must not depend on today's installs) */
                            if (best != ~0ull && dp->day - (4095u - (uint32_t)(best >> 52)) <= RP_MIRROR_STALE_DAYS &&
                                RH_STATE(e->buf.hot[(uint32_t)best]) < RS_RECOVERED) {
                                src = (uint32_t)best;
                                found = 1;
                            }
                        }
                }
                uint64_t key = rp_order_key(dp->day, prio, src);
                if (key < e->buf.cold[t].claim) e->buf.cold[t].claim = key;
                if ((uint32_t)CTL(e, REINA_L_CAND) >= e->cfg.max_candidates) {
                    set_problem(e, REINA_PROBLEM_CANDIDATE_OVERFLOW);
                    continue;
                }
                uint32_t *cd = e->buf.candidates + 4u * (uint32_t)CTL(e, REINA_L_CAND)++;
                cd[0] = t;
                cd[1] = src;
                /* a local stand-in source: its word as it stands now (before the day's bed / ICU walk) */
                cd[2] = v | ((!(src & RP_REMOTE_SRC) && (e->buf.hot[src] & RH_HASLIST)) ? 0x100u : 0u);
                cd[3] = prio;
            }
        }
}

static void run_install(Par *e, const reina_day_t *dp) {
    int C = CTL(e, REINA_L_CAND);
    for (int k = 0; k < C; k++) {
        const uint32_t *cd = e->buf.candidates + 4u * (uint32_t)k;
        if (e->buf.cold[cd[0]].claim != rp_order_key(dp->day, cd[3], cd[1])) continue;
        if (RH_STATE(e->buf.hot[cd[0]]) != RS_SUSCEPTIBLE) continue; /* duplicate record of the winner */
        int32_t src = (cd[1] & RP_REMOTE_SRC) ? -1 : (int32_t)cd[1];
        install_infection(e, cd[0], dp->day, cd[2] & 0xFFu, src, 0, dp->testing_mode, (cd[2] >> 8) & 1u);
    }
    /* tomorrow's mirror-table sizes: about twice this shard's share of today's cross-shard attempts of
     * the cell (pressure holds the sums over all shards by now), a power of two in [8, mirror_slots] */
    if (e->cfg.n_shards > 1 && !e->exact)
        for (uint32_t cell = 0; cell < REINA_MIRROR_CELLS; cell++) {
            uint32_t tot = 0;
            for (uint32_t dest = 0; dest < e->cfg.n_shards; dest++) {
                int n = e->buf.pressure[dest * REINA_MIRROR_CELLS + cell];
                tot += n > 0 ? (uint32_t)n : 0u;
            }
            const uint32_t want = 2u * ((tot + e->cfg.n_shards - 1) / e->cfg.n_shards);
            uint32_t eff = e->cfg.mirror_slots < RP_MIRROR_MIN_SLOTS ? e->cfg.mirror_slots : RP_MIRROR_MIN_SLOTS;
            while (eff < want && eff < e->cfg.mirror_slots) eff <<= 1;
            e->buf.mirror_meta[cell] = eff;
        }
}

/* Context.iterate (main.pyx:2011-2018) in the parallel formulation, as the phases between which a sharded population
 * exchanges (include/reina_hip.h: reina_step_phase) */
static void open_day(Par *e, const reina_day_t *dp) {
    if (dp->history_row) memcpy(dp->history_row, e->buf.counters, sizeof(int32_t) * REINA_COUNTER_WORDS);
    uint32_t import_base = 0;
    SC(e, REINA_S_DAY) = (int32_t)dp->day + 1;
    SC(e, REINA_S_BEDS) += dp->add_beds;
    SC(e, REINA_S_AVAILABLE_BEDS) += dp->add_beds;
    SC(e, REINA_S_ICU_UNITS) += dp->add_icu_units;
    SC(e, REINA_S_AVAILABLE_ICU) += dp->add_icu_units;
    run_imports(e, dp, 1, &import_base);
    /* Population.init_day (main.pyx:1687-1699) + Context._iterate zeroing (:1998-2000) */
    for (int i = 0; i < REINA_NR_PLACES; i++) SC(e, REINA_S_DAILY_CONTACTS + i) = 0;
    for (uint32_t a = 0; a < e->cfg.nr_ages; a++) {
        CNT(e, REINA_C_NEW_INFECTIONS, a) = 0;
        CNT(e, REINA_C_DETECTED, a) = 0;
    }
    for (int i = 0; i < REINA_MAX_VARIANTS; i++) SC(e, REINA_S_INFECTED_BY_VARIANT + i) = 0;
    SC(e, REINA_S_TOTAL_INFECTORS) = 0;
    SC(e, REINA_S_TOTAL_INFECTIONS) = 0;
    SC(e, REINA_S_EXPOSED_PER_DAY) = 0;
    CTL(e, REINA_L_WORK) = 0;
    CTL(e, REINA_L_CAND) = 0;
    CTL(e, REINA_L_HOSP) = 0;
    CTL(e, REINA_L_CONTACTS) = 0;
    CTL(e, REINA_L_HOSP_ADMIT) = 0;
    CTL(e, REINA_L_ICU_ADMIT) = 0;
    memset(e->buf.pressure, 0, sizeof(int32_t) * REINA_EXCHANGE_WORDS(e->cfg.n_shards, e->hosp_ranges));
    run_imports(e, dp, 0, &import_base);
}

int par_step_phase(Par *e, const reina_day_t *dp, int phase, void *stream) {
    (void)stream;
    if (!e->bound) return REINA_E_NOT_BOUND;
    if (dp->day >= REINA_MAX_DAYS) return REINA_E_INVALID;   /* the 12-bit day tag of rp_order_key, as the engine */
    /* the exchanges of a tracing day under exact attribution: requests at level 0, then at level 1 */
    const int xtrace = e->exact && dp->testing_mode == RT_ALL_WITH_SYMPTOMS_CT;
    switch (phase) {
    case REINA_PH_OPEN:
        open_day(e, dp);
        run_testing_level0(e, dp);
        return xtrace ? REINA_X_ALLTOALL : 0;
    case REINA_PH_TRACE:
        if (xtrace) run_trace_requests(e, dp, 0);
        run_testing_level1(e, dp);
        return xtrace ? REINA_X_ALLTOALL : 0;
    case REINA_PH_MAIN: {
        if (xtrace) run_trace_requests(e, dp, 1);
        run_vaccinations(e, dp);
        /* a sharded population's free capacity at day open and (below) its demand travel with the pressure all-reduce */
        const int32_t free_beds_open = SC(e, REINA_S_AVAILABLE_BEDS), free_icu_open = SC(e, REINA_S_AVAILABLE_ICU);
        run_scan(e, dp);
        run_contacts(e, dp);
        if (e->cfg.n_shards > 1) {
            e->buf.pressure[REINA_PRESSURE_FREE_BEDS(e->cfg.shard_rank)] = free_beds_open;
            e->buf.pressure[REINA_PRESSURE_FREE_ICU(e->cfg.shard_rank)] = free_icu_open;
            e->buf.pressure[REINA_PRESSURE_DEMAND_BEDS(e->cfg.shard_rank)] = CTL(e, REINA_L_HOSP_ADMIT);
            e->buf.pressure[REINA_PRESSURE_DEMAND_ICU(e->cfg.shard_rank)] = CTL(e, REINA_L_ICU_ADMIT);
            publish_hospital_maps(e);
            if (e->exact) {
                /* exact attribution: the four capacity words and this shard's maps ride in the trailer of every peer's segment of the
                 * mid-day exchange (no all-reduce) */
                const uint64_t *maps = exchange_maps(e, e->cfg.shard_rank);
                for (uint32_t sh = 0; sh < e->cfg.n_shards; sh++) {
                    if (sh == e->cfg.shard_rank) continue;
                    uint64_t *tr = xtrailer(e, e->buf.xsend, sh);
                    tr[0] = (uint64_t)(uint32_t)free_beds_open | ((uint64_t)(uint32_t)free_icu_open << 32);
                    tr[1] = (uint64_t)(uint32_t)CTL(e, REINA_L_HOSP_ADMIT) | ((uint64_t)(uint32_t)CTL(e, REINA_L_ICU_ADMIT) << 32);
                    for (uint32_t b = 0; b < e->hosp_ranges; b++) tr[2u + b] = maps[b];
                }
            }
        }
        if (e->exact) return REINA_X_ALLTOALL;
        return (e->cfg.n_shards > 1 || e->coll_fn) ? REINA_X_ALLREDUCE : 0;
    }
    case REINA_PH_END:
        if (e->exact) {
            /* the trailers the mid-day exchange brought: into the block an all-reduce would have filled */
            for (uint32_t sh = 0; sh < e->cfg.n_shards; sh++) {
                if (sh == e->cfg.shard_rank) continue;
                const uint64_t *tr = xtrailer(e, e->buf.xrecv, sh);
                e->buf.pressure[REINA_PRESSURE_FREE_BEDS(sh)] = (int32_t)(uint32_t)tr[0];
                e->buf.pressure[REINA_PRESSURE_FREE_ICU(sh)] = (int32_t)(uint32_t)(tr[0] >> 32);
                e->buf.pressure[REINA_PRESSURE_DEMAND_BEDS(sh)] = (int32_t)(uint32_t)tr[1];
                e->buf.pressure[REINA_PRESSURE_DEMAND_ICU(sh)] = (int32_t)(uint32_t)(tr[1] >> 32);
                uint64_t *maps = exchange_maps(e, sh);
                for (uint32_t b = 0; b < e->hosp_ranges; b++) maps[b] = tr[2u + b];
            }
        }
        run_remote(e, dp);     /* (a stand-in source's infectee-list flag: its word before the day's bed / ICU walk) */
        run_hospital(e, dp);
        run_install(e, dp);
        return e->exact ? REINA_X_ALLTOALL : 0;
    case REINA_PH_FEEDBACK:
        if (e->exact) run_feedback(e);
        return 0;
    }
    return REINA_E_INVALID;
}

/* the two halves of a day around its one all-reduce (a population without exact attribution) */
int par_step_day_begin(Par *e, const reina_day_t *dp, void *stream) {
    if (e->exact) return REINA_E_INVALID;
    for (int ph = REINA_PH_OPEN; ph <= REINA_PH_MAIN; ph++) {
        const int rc = par_step_phase(e, dp, ph, stream);
        if (rc < 0) return rc;
    }
    return 0;
}
int par_step_day_end(Par *e, const reina_day_t *dp, void *stream) {
    if (e->exact) return REINA_E_INVALID;
    for (int ph = REINA_PH_END; ph <= REINA_PH_FEEDBACK; ph++) {
        const int rc = par_step_phase(e, dp, ph, stream);
        if (rc < 0) return rc;
    }
    return 0;
}

int par_set_collective(Par *e, reina_allreduce_fn fn, void *comm) {
    e->coll_fn = fn;
    e->coll_comm = comm;
    return 0;
}
int par_set_alltoall(Par *e, reina_alltoall_fn fn, void *comm) {
    e->a2a_fn = fn;
    e->a2a_comm = comm;
    return 0;
}

int par_step_day(Par *e, const reina_day_t *dp, void *stream) {
    for (int ph = 0; ph < REINA_PH_NR; ph++) {
        const int rc = par_step_phase(e, dp, ph, stream);
        if (rc < 0) return rc;
        if ((rc & REINA_X_ALLREDUCE) && e->coll_fn &&
            e->coll_fn(e->buf.pressure, e->buf.pressure, REINA_EXCHANGE_WORDS(e->cfg.n_shards, e->hosp_ranges), 2, 0, e->coll_comm, stream) != 0)
            return REINA_E_INVALID;
        if (rc & REINA_X_ALLTOALL) {
            if (!e->a2a_fn) return REINA_E_NOT_BOUND;   /* exact attribution cannot run without its exchange */
            if (e->a2a_fn(e->buf.xsend, e->buf.xrecv, REINA_XCHG_SEG_WORDS(e->cfg.xchg_cap, e->hosp_ranges), 4, e->a2a_comm, stream) != 0) return REINA_E_INVALID;
        }
    }
    return 0;
}

int par_run_days(Par *e, const reina_day_t *days, uint32_t n, void *stream) {
    for (uint32_t k = 0; k < n; k++) {
        int rc = par_step_day(e, &days[k], stream);
        if (rc) return rc;
    }
    return 0;
}

int par_run_days_hist(Par *e, const reina_day_t *days, uint32_t n, int32_t *history_base, void *stream) {
    for (uint32_t k = 0; k < n; k++) {
        reina_day_t d = days[k];
        d.history_row = history_base ? history_base + (size_t)k * REINA_COUNTER_WORDS : NULL;
        int rc = par_step_day(e, &d, stream);
        if (rc) return rc;
    }
    return 0;
}

/* group API (include/reina_hip.h: reina_group_*): on the CPU a group is just its members stepped
 * one after another -- members share nothing, so the result is the same by construction. */
typedef struct { Par **members; uint32_t n; } ParGroup;

int par_group_create(Par **engines, uint32_t n, ParGroup **out) {
    if (!engines || !out || n == 0) return REINA_E_INVALID;
    for (uint32_t k = 0; k < n; k++)
        if (engines[k]->cfg.n_agents != engines[0]->cfg.n_agents || engines[k]->cfg.n_shards != 1) return REINA_E_INVALID;
    ParGroup *g = (ParGroup *)calloc(1, sizeof(ParGroup));
    g->members = (Par **)malloc(sizeof(Par *) * n);
    memcpy(g->members, engines, sizeof(Par *) * n);
    g->n = n;
    *out = g;
    return 0;
}

int par_group_destroy(ParGroup *g) {
    if (!g) return REINA_E_INVALID;
    free(g->members);
    free(g);
    return 0;
}

int par_group_upload_contact_tables(ParGroup *g, const reina_contact_tables_t *t, void *stream) {
    for (uint32_t k = 0; k < g->n; k++) {
        int rc = par_upload_contact_tables(g->members[k], t, stream);
        if (rc) return rc;
    }
    return 0;
}

int par_group_run_days(ParGroup *g, const reina_day_t *days, uint32_t n_days, int32_t *const *history_bases, void *stream) {
    for (uint32_t k = 0; k < g->n; k++) {
        int rc = par_run_days_hist(g->members[k], days, n_days, history_bases ? history_bases[k] : NULL, stream);
        if (rc) return rc;
    }
    return 0;
}

int par_read_counters(Par *e, int32_t *out, void *stream) {
    (void)stream;
    memcpy(out, e->buf.counters, sizeof(int32_t) * REINA_COUNTER_WORDS);
    return 0;
}
int par_read_history(Par *e, const int32_t *history, uint32_t n_rows, int32_t *out, void *stream) {
    (void)stream;
    if (n_rows) memcpy(out, history, sizeof(int32_t) * REINA_COUNTER_WORDS * (size_t)n_rows);
    memcpy(out + (size_t)n_rows * REINA_COUNTER_WORDS, e->buf.counters, sizeof(int32_t) * REINA_COUNTER_WORDS);
    return 0;
}
int par_profile_enable(Par *e, int en) { (void)e; (void)en; return 0; }
int par_profile_read(Par *e, double *a, uint64_t *b, double *c) { (void)e; *a = 0; *b = 0; *c = 0; return 0; }
int par_profile_read_kernels(Par *e, double *ms, uint64_t *n) {
    (void)e;
    for (int k = 0; k < REINA_PK_NR; k++) { ms[k] = 0; n[k] = 0; }
    return 0;
}
const char *par_last_error(void) { return g_par_error; }

/* the ABI's test hook on the host build of the primitives (include/reina_hip.h: reina_test_prims) */
int par_test_prims(int what, const uint32_t *in, uint32_t n, uint32_t *out) {
    uint32_t n_in = 0, n_out = 0;
    rp_test_prim_words(what, &n_in, &n_out);
    if (!n_in || !in || !out) return REINA_E_INVALID;
    for (uint32_t k = 0; k < n; k++) rp_test_prim(what, in + (size_t)k * n_in, out + (size_t)k * n_out);
    return 0;
}

/* ---- primitive test hooks (checked against scipy / known answers in tests/test_prims.py) ---- */
void par_test_philox(const uint32_t *key, const uint32_t *ctr, uint32_t *out) {
    rp_u4 r = rp_philox(key[0], key[1], ctr[0], ctr[1], ctr[2], ctr[3]);
    memcpy(out, r.v, 16);
}
void par_test_philox2(const uint32_t *key, const uint32_t *ctr, uint32_t *out) {
    rp_u2 r = rp_philox2(key[0], ctr[0], ctr[1]);
    memcpy(out, r.v, 8);
}
void par_test_expf(const float *x, float *y, int n) { for (int i = 0; i < n; i++) y[i] = rp_expf(x[i]); }
void par_test_logf(const float *x, float *y, int n) { for (int i = 0; i < n; i++) y[i] = rp_logf(x[i]); }
void par_test_normal(const uint32_t *r, float *y, int n) { for (int i = 0; i < n; i++) y[i] = rp_normal_from_u32(r[i]); }
void par_test_gamma(float mu, float cv, uint64_t seed, uint32_t day, uint32_t purpose, float *y, int n) {
    for (int i = 0; i < n; i++)
        y[i] = rp_gamma_mu_cv(mu, cv, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)i, day, purpose, 1);
}
/* the saturating-map algebra of the bed / ICU walk (csrc/reina_prims.h: rp_sat_*), for tests that hold it against the plain
 * definition f(x) = max(x + a, m): out = {then.a, then.m, apply(then, x), packed-and-unpacked bed map a, m, ICU map a, m} */
void par_test_sat(int a1, int m1, int a2, int m2, int x, int *out) {
    rp_sat_t f, g, fb, fc;
    f.a = a1; f.m = m1; g.a = a2; g.m = m2;
    const rp_sat_t h = rp_sat_then(f, g);
    out[0] = h.a; out[1] = h.m; out[2] = rp_sat_apply(h, x);
    rp_sat_unpack(rp_sat_pack(f, g), &fb, &fc);
    out[3] = fb.a; out[4] = fb.m; out[5] = fc.a; out[6] = fc.m;
}
/* k_day's place groups against the entry search they stand for.  The HIP library derives, per distinct contact row, the thresholds
 * at which the PLACE of the selected entry changes (reina_hip.hip: reina_upload_contact_tables -> Tables::grp; a row's entries are
 * sorted by place) and k_day finds a contact's place from five comparisons; oracle B and the contacts that can transmit search the
 * entry itself.  Restated here: the derivation and both look-ups for one row (thr non-decreasing, place = meta & 0xFF) and n draws;
 * returns the number of draws on which they disagree, -1 when the row has more than six place groups (the library then keeps the
 * full search). */
int par_test_place_groups(const uint32_t *thr, const uint32_t *meta, int cnt, const uint32_t *r0, int n) {
    uint32_t G[6] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0};
    uint32_t groups = 0, last_place = 0;
    for (int e = 0; e < cnt; e++) {
        const uint32_t place = meta[e] & 0xFFu;
        if (e == 0 || place != last_place) {
            if (e > 0 && groups <= 5) G[groups - 1] = thr[e - 1];
            if (groups < 6) G[5] |= (place * 5u) << (5u * groups);
            groups++;
            last_place = place;
        }
    }
    if (groups > 6) return -1;
    for (uint32_t q = groups; q < 6 && groups > 0; q++) G[5] |= (last_place * 5u) << (5u * q);
    int bad = 0;
    for (int k = 0; k < n; k++) {
        int l2 = 0;
        while (l2 < cnt - 1 && r0[k] >= thr[l2]) l2++;   /* first entry with r0 < threshold; none: the last one */
        const uint32_t place_entry = cnt > 0 ? (meta[l2] & 0xFFu) : 0u;
        uint32_t g = 0;
        for (int q = 0; q < 5; q++) g += r0[k] >= G[q];
        const uint32_t place_group = ((G[5] >> (5u * g)) & 31u) / 5u;
        bad += cnt > 0 && place_entry != place_group;
    }
    return bad;
}
/* rp_chance against its integer form (csrc/reina_prims.h: rp_chance_threshold; k_day tests a source's thinning bound that
 * way): n (probability bits, draw) pairs -> the number of pairs on which the two disagree */
int par_test_chance_threshold(const uint32_t *p_bits, const uint32_t *r, int n) {
    int bad = 0;
    for (int i = 0; i < n; i++) {
        const float p = rp_u2f(p_bits[i]);
        bad += (rp_chance(p, r[i]) != 0) != ((r[i] >> 8) < rp_chance_threshold(p));
    }
    return bad;
}
/* the count one given 32-bit draw yields for an age with `nrc` contacts a day (tests: the "never" encoding of the thresholds) */
int par_test_count_from_draw(float nrc, int ill, uint32_t r) {
    uint32_t row[REINA_COUNT_WORDS];
    rc_count_thresholds(nrc, row);
    return rc_count_from_draw(row, ill, r);
}
void par_test_nr_contacts(uint64_t seed, uint32_t day, float nrc, float factor, int limit, int32_t *y, int n) {
    uint32_t row[REINA_COUNT_WORDS];
    (void)limit;
    rc_count_thresholds(nrc, row);
    for (int i = 0; i < n; i++)
        y[i] = rc_count_from_draw(row, factor < 1.0f, rp_count_draw((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)i, day));
}
