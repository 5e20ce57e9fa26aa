// reina_hip.hip part: snapshots of an unsharded engine between two days (include/reina_snapshot.h; DESIGN.md "Snapshots").
// Included at the end of reina_hip.hip (it uses the host helpers and the group above); not a standalone header.
//
// An agent is recorded iff its hot word is non-zero; everything else about it is k_init's default.  Packing is three launches:
// k_snap_count (one wave per 512-agent tile: the tile's record counts of both streams by ballot), k_snap_scan (one workgroup:
// exclusive offsets of the tiles, kept in the engine's d_snap) and k_snap_pack (the same waves write their records at those
// offsets, in agent order -- the bytes do not depend on scheduling).  Unpacking is ONE launch, k_snap_unpack: a workgroup per
// tile stages the tile's records in LDS and writes every word of the tile's agents (defaults + records, both bit planes)
// into one engine, or into every member of an engine group; a few more workgroups copy the counters, control block and queues.
#include "../../include/reina_snapshot.h"

#define SNAP_TILES_PER_BLOCK 4u   // k_snap_count / k_snap_pack: 256 threads, one wave per tile
#define SNAP_UNPACK_THREADS 512   // k_snap_unpack: one thread per agent of the tile
#define SNAP_DENSE_BLOCKS 16u     // ... and these workgroups for the dense blocks (counters, control, queues)
#define SNAP_SCAN_THREADS 1024
static_assert(REINA_SNAP_TILE == 512u && REINA_SNAP_TILE == 8u * 64u, "a tile = 8 rounds of one wave = 16 words of a bit plane");
static_assert(REINA_SNAP_RECORD_WORDS * 4u == sizeof(reina_cold_t) && REINA_INLINE_INFECTEES == 8, "32-byte records");
static_assert(REINA_L_QUEUE1 == REINA_L_QUEUE0 + 1 && REINA_L_LEVEL1 == REINA_L_QUEUE0 + 2, "queue lengths side by side");

// word offsets of an image's sections
struct SnapLayout {
    uint32_t n_tiles;
    uint64_t tb, ts, pad, rb, rs, q, words;
};
static SnapLayout snap_layout(uint32_t n_agents, uint64_t n_base, uint64_t n_slot, const uint32_t qlen[3]) {
    SnapLayout l;
    l.n_tiles = (uint32_t)(((uint64_t)n_agents + REINA_SNAP_TILE - 1u) / REINA_SNAP_TILE);
    l.tb = REINA_SNAP_HEADER_WORDS + REINA_COUNTER_WORDS + REINA_L_NR;
    l.ts = l.tb + l.n_tiles + 1u;
    l.pad = l.ts + l.n_tiles + 1u;
    l.rb = (l.pad + 7u) & ~(uint64_t)7u;   // records on 32-byte boundaries
    l.rs = l.rb + REINA_SNAP_RECORD_WORDS * n_base;
    l.q = l.rs + REINA_SNAP_RECORD_WORDS * n_slot;
    l.words = l.q + (uint64_t)qlen[0] + qlen[1] + qlen[2];
    return l;
}

// ---------------------------------------------------------------------------------------------
// k_snap_count: per tile, the agents with a record (hot != 0) and those of them with inline infectees (slot 0 used: the slots
// are filled in rank order).  cnt[0, n_tiles) base, cnt[n_tiles + 1, 2 n_tiles + 1) slots.
__global__ __launch_bounds__(256) void k_snap_count(const uint32_t *__restrict__ hot, const int32_t *__restrict__ infectees,
                                                    uint32_t n_agents, uint32_t n_tiles, uint32_t *__restrict__ cnt) {
    const uint32_t tile = blockIdx.x * SNAP_TILES_PER_BLOCK + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;   // (whole waves)
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t nb = 0, ns = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8u; j++) {
        const uint32_t i = tile * REINA_SNAP_TILE + j * 64u + lane;
        const uint32_t h = i < n_agents ? hot[i] : 0u;
        const bool rec = h != 0u;
        const bool sl = rec && infectees[(size_t)i * REINA_INLINE_INFECTEES] != -1;
        nb += (uint32_t)__popcll(__ballot(rec));
        ns += (uint32_t)__popcll(__ballot(sl));
    }
    if (lane == 0) {
        cnt[tile] = nb;
        cnt[n_tiles + 1u + tile] = ns;
    }
}

// k_snap_scan: one workgroup turns both count arrays into exclusive offsets in place; entry n_tiles = the stream's total.
__global__ __launch_bounds__(SNAP_SCAN_THREADS) void k_snap_scan(uint32_t *cnt, uint32_t n_tiles) {
    __shared__ uint32_t sb[SNAP_SCAN_THREADS], ss[SNAP_SCAN_THREADS];
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (n_tiles + SNAP_SCAN_THREADS - 1u) / SNAP_SCAN_THREADS;
    const uint32_t lo = tid * per, hi = lo + per < n_tiles ? lo + per : n_tiles;
    uint32_t *cb = cnt, *cs = cnt + n_tiles + 1u;
    uint32_t tb = 0, ts = 0;
    for (uint32_t k = lo; k < hi; k++) {
        tb += cb[k];
        ts += cs[k];
    }
    sb[tid] = tb;
    ss[tid] = ts;
    __syncthreads();
    for (uint32_t off = 1; off < SNAP_SCAN_THREADS; off <<= 1) {
        const uint32_t vb = tid >= off ? sb[tid - off] : 0u, vs = tid >= off ? ss[tid - off] : 0u;
        __syncthreads();
        sb[tid] += vb;
        ss[tid] += vs;
        __syncthreads();
    }
    uint32_t ob = sb[tid] - tb, os = ss[tid] - ts;
    for (uint32_t k = lo; k < hi; k++) {
        const uint32_t b = cb[k], s = cs[k];
        cb[k] = ob;
        cs[k] = os;
        ob += b;
        os += s;
    }
    if (tid == SNAP_SCAN_THREADS - 1u) {
        cb[n_tiles] = sb[tid];
        cs[n_tiles] = ss[tid];
    }
}

// k_snap_pack: the records of every tile at the tile's offsets, in agent order.  out: the image; rb / rs: word offsets of the
// two record streams.
__global__ __launch_bounds__(256) void k_snap_pack(const uint32_t *__restrict__ hot, const reina_cold_t *__restrict__ cold,
                                                   const int32_t *__restrict__ infectees, const uint32_t *__restrict__ offs,
                                                   uint32_t n_agents, uint32_t n_tiles, uint32_t *__restrict__ out,
                                                   uint64_t rb, uint64_t rs) {
    const uint32_t tile = blockIdx.x * SNAP_TILES_PER_BLOCK + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t below = (1ull << lane) - 1ull;
    uint32_t pb = offs[tile], ps = offs[n_tiles + 1u + tile];
    for (uint32_t j = 0; j < 8u; j++) {
        const uint32_t i = tile * REINA_SNAP_TILE + j * 64u + lane;
        const uint32_t h = i < n_agents ? hot[i] : 0u;
        const bool rec = h != 0u;
        const v4u_ *slots = reinterpret_cast<const v4u_ *>(infectees + (size_t)i * REINA_INLINE_INFECTEES);
        v4u_ s0 = {0u, 0u, 0u, 0u};
        if (rec) s0 = slots[0];
        const bool sl = rec && s0.x != 0xFFFFFFFFu;
        const uint64_t mb = __ballot(rec), ms = __ballot(sl);
        if (rec) {
            const v4u_ *c = reinterpret_cast<const v4u_ *>(&cold[i]);
            const v4u_ c0 = c[0], c1 = c[1];   // claim (not kept), infector, n_infected | onset, vacc_day, first_infectee, next_sibling
            v4u_ a;
            a.x = i | (sl ? 0x80000000u : 0u);
            a.y = h;
            a.z = c0.z;
            a.w = c0.w;
            v4u_ *o = reinterpret_cast<v4u_ *>(out + rb + (uint64_t)(pb + (uint32_t)__popcll(mb & below)) * REINA_SNAP_RECORD_WORDS);
            o[0] = a;
            o[1] = c1;
        }
        if (sl) {
            v4u_ *o = reinterpret_cast<v4u_ *>(out + rs + (uint64_t)(ps + (uint32_t)__popcll(ms & below)) * REINA_SNAP_RECORD_WORDS);
            o[0] = s0;
            o[1] = slots[1];
        }
        pb += (uint32_t)__popcll(mb);
        ps += (uint32_t)__popcll(ms);
    }
}

struct SnapUnpackArgs {
    const uint32_t *in;   // the image (device)
    uint64_t tb, ts, rb, rs, q;
    uint32_t n_agents, n_tiles, n_base, n_slot;
    uint32_t qlen[3];
    uint32_t members, members_per_block;
};

// k_snap_unpack: blocks [0, n_tiles) one tile each, blocks [n_tiles, n_tiles + SNAP_DENSE_BLOCKS) the dense blocks.
// GROUP: members [blockIdx.y * members_per_block, ...) of the array M_ (read through the constant address space, as
// MEMBER_OF_LAUNCH does); otherwise the one engine `one_`.  Every store is bounded by the engine's own sizes, whatever the
// image's tile tables say (the host has validated the header; a tile whose offsets are out of range restores defaults).
template <bool GROUP>
__global__ __launch_bounds__(SNAP_UNPACK_THREADS) void k_snap_unpack(const MemberRef *M_, const MemberRef one_, const SnapUnpackArgs a) {
    __shared__ uint32_t rw[REINA_SNAP_TILE * REINA_SNAP_RECORD_WORDS];   // the tile's base records
    __shared__ uint32_t sw[REINA_SNAP_TILE * REINA_SNAP_RECORD_WORDS];   // ... and slot records
    __shared__ int32_t rmap[REINA_SNAP_TILE], smap[REINA_SNAP_TILE];      // agent of the tile -> its records, -1 = none
    __shared__ uint32_t wave_flagged[SNAP_UNPACK_THREADS / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t m0 = GROUP ? blockIdx.y * a.members_per_block : 0u;
    const uint32_t m1 = GROUP ? (m0 + a.members_per_block < a.members ? m0 + a.members_per_block : a.members) : 1u;
    if (blockIdx.x >= a.n_tiles) {
        // counters and control (contiguous behind the header), then the three queues
        const uint32_t dense = REINA_COUNTER_WORDS + REINA_L_NR;
        const uint64_t total = (uint64_t)dense + a.qlen[0] + a.qlen[1] + a.qlen[2];
        const uint64_t stride = (uint64_t)SNAP_DENSE_BLOCKS * SNAP_UNPACK_THREADS;
        for (uint32_t m = m0; m < m1; m++) {
            MemberRef ref;
            if (GROUP) member_from_constant(&ref, M_ + m);
            const reina_buffers_t &B = GROUP ? ref.B : one_.B;
            for (uint64_t w = (uint64_t)(blockIdx.x - a.n_tiles) * SNAP_UNPACK_THREADS + tid; w < total; w += stride) {
                if (w < REINA_COUNTER_WORDS) {
                    B.counters[w] = (int32_t)a.in[REINA_SNAP_HEADER_WORDS + w];
                } else if (w < dense) {
                    B.control[w - REINA_COUNTER_WORDS] = (int32_t)a.in[REINA_SNAP_HEADER_WORDS + w];
                } else {
                    const uint64_t k = w - dense;
                    const uint32_t v = a.in[a.q + k];
                    if (k < a.qlen[0]) B.queue0[k] = v;
                    else if (k < (uint64_t)a.qlen[0] + a.qlen[1]) B.queue1[k - a.qlen[0]] = v;
                    else B.level1[k - a.qlen[0] - a.qlen[1]] = v;
                }
            }
        }
        return;
    }
    const uint32_t t = blockIdx.x;
    const uint32_t first = t * REINA_SNAP_TILE;
    rmap[tid] = -1;
    smap[tid] = -1;
    const uint32_t b0 = a.in[a.tb + t], b1 = a.in[a.tb + t + 1u], s0 = a.in[a.ts + t], s1 = a.in[a.ts + t + 1u];
    const bool ok = b0 <= b1 && b1 - b0 <= REINA_SNAP_TILE && b1 <= a.n_base && s0 <= s1 && s1 - s0 <= REINA_SNAP_TILE && s1 <= a.n_slot;
    const uint32_t nb = ok ? b1 - b0 : 0u, ns = ok ? s1 - s0 : 0u;
    __syncthreads();
    bool flagged = false;
    uint32_t local = 0;
    if (tid < nb) {
        const v4u_ *r = reinterpret_cast<const v4u_ *>(a.in + a.rb + (uint64_t)(b0 + tid) * REINA_SNAP_RECORD_WORDS);
        const v4u_ r0 = r[0], r1 = r[1];
        v4u_ *d = reinterpret_cast<v4u_ *>(&rw[tid * REINA_SNAP_RECORD_WORDS]);
        d[0] = r0;
        d[1] = r1;
        const uint32_t idx = r0.x & 0x7FFFFFFFu;
        if (idx >= first && idx - first < REINA_SNAP_TILE && idx < a.n_agents) {
            local = idx - first;
            rmap[local] = (int32_t)tid;
            flagged = (r0.x >> 31) != 0u;
        }
    }
    // the slot records follow the flagged base records in order: rank among them = ballot prefix + the waves before
    const uint64_t mf = __ballot(flagged);
    if (lane == 0) wave_flagged[wave] = (uint32_t)__popcll(mf);
    __syncthreads();
    uint32_t rank = (uint32_t)__popcll(mf & ((1ull << lane) - 1ull));
    for (uint32_t w = 0; w < wave; w++) rank += wave_flagged[w];
    if (flagged && rank < ns) {
        const v4u_ *r = reinterpret_cast<const v4u_ *>(a.in + a.rs + (uint64_t)(s0 + rank) * REINA_SNAP_RECORD_WORDS);
        v4u_ *d = reinterpret_cast<v4u_ *>(&sw[rank * REINA_SNAP_RECORD_WORDS]);
        d[0] = r[0];
        d[1] = r[1];
        smap[local] = (int32_t)rank;
    }
    __syncthreads();
    // this thread's agent: its words as k_init leaves them, overlaid with its records
    const uint32_t i = first + tid;
    const int32_t r = rmap[tid], sr = smap[tid];
    uint32_t h = 0u;
    v4u_ lo = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u}, hi = {0u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    v4u_ ia = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, ib = ia;
    if (r >= 0) {
        const v4u_ *q = reinterpret_cast<const v4u_ *>(&rw[r * REINA_SNAP_RECORD_WORDS]);
        const v4u_ q0 = q[0];
        h = q0.y;
        lo.z = q0.z;
        lo.w = q0.w;
        hi = q[1];
    }
    if (sr >= 0) {
        const v4u_ *q = reinterpret_cast<const v4u_ *>(&sw[sr * REINA_SNAP_RECORD_WORDS]);
        ia = q[0];
        ib = q[1];
    }
    const uint64_t act = __ballot((h & RH_ACTIVE) != 0u), inf = __ballot(RH_STATE(h) != 0u);
    const size_t bw = (size_t)t * 16u + wave * 2u;   // the wave's 64 agents = two words of a bit plane
    for (uint32_t m = m0; m < m1; m++) {
        MemberRef ref;
        if (GROUP) member_from_constant(&ref, M_ + m);
        const reina_buffers_t &B = GROUP ? ref.B : one_.B;
        if (i < a.n_agents) {
            B.hot[i] = h;
            v4u_ *c = reinterpret_cast<v4u_ *>(&B.cold[i]);
            c[0] = lo;
            c[1] = hi;
            v4u_ *s = reinterpret_cast<v4u_ *>(B.infectees + (size_t)i * REINA_INLINE_INFECTEES);
            s[0] = ia;
            s[1] = ib;
        }
        if (lane == 0) {
            B.active_bits[bw] = (uint32_t)act;
            B.active_bits[bw + 1u] = (uint32_t)(act >> 32);
            B.infected_bits[bw] = (uint32_t)inf;
            B.infected_bits[bw + 1u] = (uint32_t)(inf >> 32);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// host side

static uint64_t snap_fnv1a(const void *p, size_t n) {
    const unsigned char *b = static_cast<const unsigned char *>(p);
    uint64_t h = 14695981039346656037ull;   // FNV-1a 64: offset basis 0xCBF29CE484222325, prime 2^40 + 2^8 + 0xB3
    for (size_t k = 0; k < n; k++) {
        h ^= b[k];
        h *= 1099511628211ull;
    }
    return h;
}

static int snap_engine_ok(const reina_engine_t *e) {
    if (!e) return REINA_E_INVALID;
    if (!e->bound) return REINA_E_NOT_BOUND;
    if (e->cfg.n_shards > 1 || e->exact) return refuse("snapshots are taken of, and restored into, unsharded engines only");
    return REINA_OK;
}

// the header an image of engine `e` with these counts carries
static void snap_header(const reina_engine_t *e, uint32_t n_base, uint32_t n_slot, const uint32_t qlen[3], uint32_t *h) {
    const SnapLayout l = snap_layout(e->cfg.n_agents, n_base, n_slot, qlen);
    std::memset(h, 0, REINA_SNAP_HEADER_WORDS * 4u);
    h[REINA_SNAP_H_MAGIC] = REINA_SNAP_MAGIC;
    h[REINA_SNAP_H_VERSION] = REINA_SNAPSHOT_VERSION;
    h[REINA_SNAP_H_N_AGENTS] = e->cfg.n_agents;
    h[REINA_SNAP_H_NR_AGES] = e->cfg.nr_ages;
    h[REINA_SNAP_H_NR_VARIANTS] = e->cfg.nr_variants;
    h[REINA_SNAP_H_N_TILES] = l.n_tiles;
    h[REINA_SNAP_H_N_BASE] = n_base;
    h[REINA_SNAP_H_N_SLOT] = n_slot;
    h[REINA_SNAP_H_FLAGS] = e->testing_ever ? REINA_SNAP_FLAG_TESTING_EVER : 0u;
    for (int k = 0; k < 3; k++) h[REINA_SNAP_H_LEN_Q0 + k] = qlen[k];
    const uint64_t ah = snap_fnv1a(e->cfg.age_start, sizeof(e->cfg.age_start));
    const uint64_t dh = snap_fnv1a(&e->h_params.dis, sizeof(reina_disease_t));
    const uint64_t bytes = l.words * 4u;
    h[REINA_SNAP_H_AGES_HASH] = (uint32_t)ah;
    h[REINA_SNAP_H_AGES_HASH + 1] = (uint32_t)(ah >> 32);
    h[REINA_SNAP_H_DISEASE_HASH] = (uint32_t)dh;
    h[REINA_SNAP_H_DISEASE_HASH + 1] = (uint32_t)(dh >> 32);
    h[REINA_SNAP_H_BYTES] = (uint32_t)bytes;
    h[REINA_SNAP_H_BYTES + 1] = (uint32_t)(bytes >> 32);
}

// an image's header against engine `e`: the same population, variants and disease, counts within the engine's buffers
static int snap_validate(const reina_engine_t *e, const uint32_t *h, SnapLayout *l) {
    if (int rc = snap_engine_ok(e)) return rc;
    const uint32_t N = e->cfg.n_agents;
    const uint32_t qlen[3] = {h[REINA_SNAP_H_LEN_Q0], h[REINA_SNAP_H_LEN_Q1], h[REINA_SNAP_H_LEN_L1]};
    if (h[REINA_SNAP_H_MAGIC] != REINA_SNAP_MAGIC) return refuse("not a snapshot image (magic)");
    if (h[REINA_SNAP_H_VERSION] != REINA_SNAPSHOT_VERSION) return refuse("snapshot format version differs from the library's");
    if (h[REINA_SNAP_H_N_AGENTS] != N || h[REINA_SNAP_H_NR_AGES] != e->cfg.nr_ages) return refuse("snapshot of another population");
    if (h[REINA_SNAP_H_NR_VARIANTS] != e->cfg.nr_variants) return refuse("snapshot with another number of variants");
    if (h[REINA_SNAP_H_N_BASE] > N || h[REINA_SNAP_H_N_SLOT] > h[REINA_SNAP_H_N_BASE]) return refuse("snapshot record counts out of range");
    if (qlen[0] > e->cfg.max_queue || qlen[1] > e->cfg.max_queue || qlen[2] > e->cfg.max_queue) return refuse("snapshot queue longer than the engine's queues");
    uint32_t want[REINA_SNAP_HEADER_WORDS];
    snap_header(e, h[REINA_SNAP_H_N_BASE], h[REINA_SNAP_H_N_SLOT], qlen, want);
    if (std::memcmp(&h[REINA_SNAP_H_AGES_HASH], &want[REINA_SNAP_H_AGES_HASH], 8) != 0) return refuse("snapshot of another population (age structure)");
    if (std::memcmp(&h[REINA_SNAP_H_DISEASE_HASH], &want[REINA_SNAP_H_DISEASE_HASH], 8) != 0) return refuse("snapshot of another disease");
    if (h[REINA_SNAP_H_N_TILES] != want[REINA_SNAP_H_N_TILES] || h[REINA_SNAP_H_BYTES] != want[REINA_SNAP_H_BYTES] || h[REINA_SNAP_H_BYTES + 1] != want[REINA_SNAP_H_BYTES + 1])
        return refuse("snapshot image size does not match its header");
    *l = snap_layout(N, h[REINA_SNAP_H_N_BASE], h[REINA_SNAP_H_N_SLOT], qlen);
    return REINA_OK;
}

static int snap_read_header(const void *dev_in, uint32_t *h, hipStream_t s) {
    HIP_CHECK(hipMemcpyAsync(h, dev_in, REINA_SNAP_HEADER_WORDS * 4u, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    return REINA_OK;
}

static SnapUnpackArgs snap_unpack_args(const uint32_t *h, const SnapLayout &l, const void *dev_in) {
    SnapUnpackArgs a;
    a.in = static_cast<const uint32_t *>(dev_in);
    a.tb = l.tb;
    a.ts = l.ts;
    a.rb = l.rb;
    a.rs = l.rs;
    a.q = l.q;
    a.n_agents = h[REINA_SNAP_H_N_AGENTS];
    a.n_tiles = l.n_tiles;
    a.n_base = h[REINA_SNAP_H_N_BASE];
    a.n_slot = h[REINA_SNAP_H_N_SLOT];
    for (int k = 0; k < 3; k++) a.qlen[k] = h[REINA_SNAP_H_LEN_Q0 + k];
    a.members = 1;
    a.members_per_block = 1;
    return a;
}

extern "C" {

int reina_snapshot_version(void) { return REINA_SNAPSHOT_VERSION; }

int reina_snap_measure(reina_engine_t *e, uint64_t *bytes, void *stream) {
    if (int rc = snap_engine_ok(e)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t N = e->cfg.n_agents;
    const uint32_t T = (N + REINA_SNAP_TILE - 1u) / REINA_SNAP_TILE;
    if (!e->d_snap) HIP_CHECK(hipMalloc(&e->d_snap, 2u * ((size_t)T + 1u) * 4u));
    hipLaunchKernelGGL(k_snap_count, dim3((T + SNAP_TILES_PER_BLOCK - 1u) / SNAP_TILES_PER_BLOCK), dim3(256), 0, s,
                       e->buf.hot, e->buf.infectees, N, T, e->d_snap);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_snap_scan, dim3(1), dim3(SNAP_SCAN_THREADS), 0, s, e->d_snap, T);
    HIP_CHECK(hipGetLastError());
    uint32_t tot[2];
    int32_t qlen[3];
    HIP_CHECK(hipMemcpyAsync(&tot[0], e->d_snap + T, 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(&tot[1], e->d_snap + 2u * T + 1u, 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(qlen, e->buf.control + REINA_L_QUEUE0, sizeof(qlen), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    for (int k = 0; k < 3; k++) {
        if (qlen[k] < 0 || (uint32_t)qlen[k] > e->cfg.max_queue) return refuse("a queue length of the control block is out of range");
        e->snap_qlen[k] = (uint32_t)qlen[k];
    }
    e->snap_total[0] = tot[0];
    e->snap_total[1] = tot[1];
    if (bytes) *bytes = snap_layout(N, tot[0], tot[1], e->snap_qlen).words * 4u;
    return REINA_OK;
}

int reina_snap_pack(reina_engine_t *e, void *dev_out, uint64_t cap, void *stream) {
    if (!dev_out || ((uintptr_t)dev_out & 15u)) return refuse("reina_snap_pack: the output must be a 16-byte aligned device buffer");
    uint64_t bytes = 0;
    if (int rc = reina_snap_measure(e, &bytes, stream)) return rc;
    if (cap < bytes) return refuse("reina_snap_pack: output buffer smaller than the measured image");
    hipStream_t s = (hipStream_t)stream;
    const uint32_t N = e->cfg.n_agents;
    const SnapLayout l = snap_layout(N, e->snap_total[0], e->snap_total[1], e->snap_qlen);
    uint32_t *out = static_cast<uint32_t *>(dev_out);
    uint32_t h[REINA_SNAP_HEADER_WORDS];
    snap_header(e, e->snap_total[0], e->snap_total[1], e->snap_qlen, h);
    HIP_CHECK(hipMemcpyAsync(out, h, sizeof(h), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(out + REINA_SNAP_HEADER_WORDS, e->buf.counters, REINA_COUNTER_WORDS * 4u, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(out + REINA_SNAP_HEADER_WORDS + REINA_COUNTER_WORDS, e->buf.control, REINA_L_NR * 4u, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(out + l.tb, e->d_snap, 2u * ((size_t)l.n_tiles + 1u) * 4u, hipMemcpyDeviceToDevice, s));   // (both tables, side by side)
    if (l.rb > l.pad) HIP_CHECK(hipMemsetAsync(out + l.pad, 0, (l.rb - l.pad) * 4u, s));
    hipLaunchKernelGGL(k_snap_pack, dim3((l.n_tiles + SNAP_TILES_PER_BLOCK - 1u) / SNAP_TILES_PER_BLOCK), dim3(256), 0, s,
                       e->buf.hot, e->buf.cold, e->buf.infectees, e->d_snap, N, l.n_tiles, out, l.rb, l.rs);
    HIP_CHECK(hipGetLastError());
    uint64_t q = l.q;
    const uint32_t *queues[3] = {e->buf.queue0, e->buf.queue1, e->buf.level1};
    for (int k = 0; k < 3; k++) {
        if (e->snap_qlen[k]) HIP_CHECK(hipMemcpyAsync(out + q, queues[k], (size_t)e->snap_qlen[k] * 4u, hipMemcpyDeviceToDevice, s));
        q += e->snap_qlen[k];
    }
    HIP_CHECK(hipStreamSynchronize(s));   // (the header's staging copy is a host array of this frame)
    return REINA_OK;
}

int reina_snap_unpack(reina_engine_t *e, const void *dev_in, void *stream) {
    if (int rc = snap_engine_ok(e)) return rc;
    if (!dev_in || ((uintptr_t)dev_in & 15u)) return refuse("reina_snap_unpack: the image must be a 16-byte aligned device buffer");
    hipStream_t s = (hipStream_t)stream;
    uint32_t h[REINA_SNAP_HEADER_WORDS];
    if (int rc = snap_read_header(dev_in, h, s)) return rc;
    SnapLayout l;
    if (int rc = snap_validate(e, h, &l)) return rc;
    const SnapUnpackArgs a = snap_unpack_args(h, l, dev_in);
    hipLaunchKernelGGL((k_snap_unpack<false>), dim3(l.n_tiles + SNAP_DENSE_BLOCKS, 1), dim3(SNAP_UNPACK_THREADS), 0, s,
                       e->d_ref, e->h_ref, a);
    HIP_CHECK(hipGetLastError());
    e->testing_ever = (h[REINA_SNAP_H_FLAGS] & REINA_SNAP_FLAG_TESTING_EVER) != 0u;
    return REINA_OK;
}

int reina_group_snap_unpack(reina_group_t *g, const void *dev_in, void *stream) {
    if (!g || g->members.empty()) return REINA_E_INVALID;
    if (!dev_in || ((uintptr_t)dev_in & 15u)) return refuse("reina_group_snap_unpack: the image must be a 16-byte aligned device buffer");
    hipStream_t s = (hipStream_t)stream;
    uint32_t h[REINA_SNAP_HEADER_WORDS];
    if (int rc = snap_read_header(dev_in, h, s)) return rc;
    SnapLayout l;
    for (auto m : g->members)
        if (int rc = snap_validate(m, h, &l)) return rc;
    const uint32_t K = (uint32_t)g->members.size();
    SnapUnpackArgs a = snap_unpack_args(h, l, dev_in);
    // each tile's records are read once per chunk of members: all members in one chunk unless the tiles alone cannot fill the
    // chip (then a few chunks along blockIdx.y)
    uint32_t chunks = (4u * g->members[0]->n_cus + l.n_tiles - 1u) / l.n_tiles;
    if (chunks < 1u) chunks = 1u;
    if (chunks > K) chunks = K;
    a.members = K;
    a.members_per_block = (K + chunks - 1u) / chunks;
    chunks = (K + a.members_per_block - 1u) / a.members_per_block;
    hipLaunchKernelGGL((k_snap_unpack<true>), dim3(l.n_tiles + SNAP_DENSE_BLOCKS, chunks), dim3(SNAP_UNPACK_THREADS), 0, s,
                       g->d_refs, g->h_refs[0], a);
    HIP_CHECK(hipGetLastError());
    const bool tested = (h[REINA_SNAP_H_FLAGS] & REINA_SNAP_FLAG_TESTING_EVER) != 0u;
    for (auto m : g->members) m->testing_ever = tested;
    return REINA_OK;
}

}  // extern "C"
