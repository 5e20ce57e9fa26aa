// reina_hip.hip part: the particle filter's in-group clone (include/reina_filter.h; DESIGN.md "Particle filter").
// Included at the end of reina_hip.hip (it uses the host helpers and the group above); not a standalone header.
//
// ONE launch, k_group_clone, moves the carried state of every (dst, src) pair: blockIdx.y = pair, blockIdx.x = four
// 512-agent tiles (one wave each) or, past the tiles, one of CLONE_DENSE_BLOCKS workgroups of the dense blocks (counters,
// control, the queues up to the source's lengths, read from its control block on the device).  A wave streams both members'
// hot words and moves only what differs: the 64-byte record (cold + slots) of every agent the source has recorded, k_init's
// defaults where only the destination has one; agents susceptible in both are not touched.  The member table is the
// group's, read through the constant address space; the pair list travels as the kernel argument.
#include "../../include/reina_filter.h"

#define CLONE_THREADS 256
#define CLONE_TILES_PER_BLOCK 4u   // one wave per tile
#define CLONE_DENSE_BLOCKS 4u
static_assert(REINA_BITS_WORDS(1) == 32u && REINA_INLINE_INFECTEES == 8, "a tile = 16 words of a bit plane, slots = 32 bytes");

struct ClonePairs {
    uint32_t n_agents, n_tiles, max_queue, n;
    uint32_t p[REINA_CLONE_MAX_PAIRS];   // dst | src << 16 (a group has at most 65535 members)
};
static_assert(sizeof(ClonePairs) + sizeof(void *) <= 3712u, "the kernel argument stays well inside 4 KiB");

__global__ __launch_bounds__(CLONE_THREADS) void k_group_clone(const MemberRef *M_, const ClonePairs a) {
    const uint32_t pr = a.p[blockIdx.y];
    MemberRef dref, sref;
    member_from_constant(&dref, M_ + (pr & 0xFFFFu));
    member_from_constant(&sref, M_ + (pr >> 16));
    const reina_buffers_t &D = dref.B, &S = sref.B;
    const uint32_t tile_blocks = (a.n_tiles + CLONE_TILES_PER_BLOCK - 1u) / CLONE_TILES_PER_BLOCK;
    if (blockIdx.x >= tile_blocks) {
        // counters and control, then the three queues up to the source's lengths (the source is never a destination: its
        // control block is not written by this launch)
        uint32_t qlen[3];
        for (int k = 0; k < 3; k++) {
            const int32_t l = S.control[REINA_L_QUEUE0 + k];
            qlen[k] = l < 0 ? 0u : ((uint32_t)l > a.max_queue ? a.max_queue : (uint32_t)l);
        }
        const uint32_t dense = REINA_COUNTER_WORDS + REINA_L_NR;
        const uint64_t total = (uint64_t)dense + qlen[0] + qlen[1] + qlen[2];
        const uint64_t stride = (uint64_t)CLONE_DENSE_BLOCKS * CLONE_THREADS;
        for (uint64_t w = (uint64_t)(blockIdx.x - tile_blocks) * CLONE_THREADS + threadIdx.x; w < total; w += stride) {
            if (w < REINA_COUNTER_WORDS) {
                D.counters[w] = S.counters[w];
            } else if (w < dense) {
                D.control[w - REINA_COUNTER_WORDS] = S.control[w - REINA_COUNTER_WORDS];
            } else {
                const uint64_t k = w - dense;
                if (k < qlen[0]) D.queue0[k] = S.queue0[k];
                else if (k < (uint64_t)qlen[0] + qlen[1]) D.queue1[k - qlen[0]] = S.queue1[k - qlen[0]];
                else D.level1[k - qlen[0] - qlen[1]] = S.level1[k - qlen[0] - qlen[1]];
            }
        }
        return;
    }
    const uint32_t tile = blockIdx.x * CLONE_TILES_PER_BLOCK + (threadIdx.x >> 6);
    if (tile >= a.n_tiles) return;   // (whole waves)
    const uint32_t lane = threadIdx.x & 63u;
    const v4u_ lo_def = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u}, hi_def = {0u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    const v4u_ none = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
#pragma unroll 2
    for (uint32_t j = 0; j < 8u; j++) {
        const uint32_t i = tile * 512u + j * 64u + lane;
        if (i >= a.n_agents) break;
        const uint32_t sh = S.hot[i], dh = D.hot[i];
        v4u_ *dc = reinterpret_cast<v4u_ *>(&D.cold[i]);
        v4u_ *ds = reinterpret_cast<v4u_ *>(D.infectees + (size_t)i * REINA_INLINE_INFECTEES);
        if (sh != 0u) {
            const v4u_ *sc = reinterpret_cast<const v4u_ *>(&S.cold[i]);
            const v4u_ *ss = reinterpret_cast<const v4u_ *>(S.infectees + (size_t)i * REINA_INLINE_INFECTEES);
            const v4u_ c0 = sc[0], c1 = sc[1], s0 = ss[0], s1 = ss[1];
            dc[0] = c0;
            dc[1] = c1;
            ds[0] = s0;
            ds[1] = s1;
        } else if (dh != 0u) {
            dc[0] = lo_def;
            dc[1] = hi_def;
            ds[0] = none;
            ds[1] = none;
        }
        if (sh != dh) D.hot[i] = sh;
    }
    // the tile's 16 words of each bit plane
    if (lane < 16u) {
        const size_t w = (size_t)tile * 16u + lane;
        D.active_bits[w] = S.active_bits[w];
        D.infected_bits[w] = S.infected_bits[w];
    }
}

// what both clones share (reina_group_clone, and reina_group_txlog_clone of k_filter_log.inc): the checks of a pair list and
// the launches per chunk of REINA_CLONE_MAX_PAIRS pairs.  `what` names the entry point in the messages.  With a log, its
// launch is queued ahead of the state's in every chunk: it reads the destinations' hot words, which k_group_clone overwrites.
struct reina_txlog;
static int txlog_clone_launch(reina_txlog *l, const MemberRef *d_refs, uint32_t tile_blocks, const ClonePairs &a, hipStream_t s);   // (k_filter_log.inc)

static int group_clone_pairs(reina_group_t *g, reina_txlog *log, const uint32_t *pairs, uint32_t n_pairs, void *stream, const char *what) {
    if (!g || g->members.empty()) return REINA_E_INVALID;
    if (n_pairs == 0) return REINA_OK;
    const std::string w(what);
    if (!pairs) return refuse(w + ": no pair list");
    const uint32_t K = (uint32_t)g->members.size();
    // every check before anything is queued: a refused list leaves every member untouched
    std::vector<uint8_t> role(K, 0);   // bit 0: a destination, bit 1: a source
    for (uint32_t j = 0; j < n_pairs; j++) {
        const uint32_t dst = pairs[2 * j], src = pairs[2 * j + 1];
        if (dst >= K || src >= K) return refuse(w + ": a member index is out of range");
        if (role[dst] & 1u) return refuse(w + ": a destination appears twice");
        role[dst] |= 1u;
        role[src] |= 2u;
    }
    for (uint32_t m = 0; m < K; m++) {
        if (role[m] == 3u) return refuse(w + ": a source is also a destination");
    }
    uint32_t max_queue = g->members[0]->cfg.max_queue;
    for (uint32_t j = 0; j < n_pairs; j++) {
        const reina_engine_t *d = g->members[pairs[2 * j]], *s = g->members[pairs[2 * j + 1]];
        if (d->testing_ever != s->testing_ever) return refuse(w + ": the members' testing_ever flags differ (they ran different plans)");
    }
    for (auto m : g->members) {
        if (!m->bound) return REINA_E_NOT_BOUND;
        if (m->cfg.max_queue < max_queue) max_queue = m->cfg.max_queue;
    }
    hipStream_t s = (hipStream_t)stream;
    ClonePairs a;
    a.n_agents = g->members[0]->cfg.n_agents;
    a.n_tiles = (a.n_agents + 511u) / 512u;
    a.max_queue = max_queue;
    const uint32_t tile_blocks = (a.n_tiles + CLONE_TILES_PER_BLOCK - 1u) / CLONE_TILES_PER_BLOCK;
    for (uint32_t j0 = 0; j0 < n_pairs; j0 += REINA_CLONE_MAX_PAIRS) {
        a.n = n_pairs - j0 < REINA_CLONE_MAX_PAIRS ? n_pairs - j0 : REINA_CLONE_MAX_PAIRS;
        for (uint32_t j = 0; j < a.n; j++) a.p[j] = pairs[2 * (j0 + j)] | pairs[2 * (j0 + j) + 1] << 16;
        if (log)
            if (int rc = txlog_clone_launch(log, g->d_refs, tile_blocks, a, s)) return rc;
        hipLaunchKernelGGL(k_group_clone, dim3(tile_blocks + CLONE_DENSE_BLOCKS, a.n), dim3(CLONE_THREADS), 0, s, g->d_refs, a);
        HIP_CHECK(hipGetLastError());
    }
    return REINA_OK;
}

extern "C" {

int reina_filter_version(void) { return REINA_FILTER_VERSION; }

int reina_group_clone(reina_group_t *g, const uint32_t *pairs, uint32_t n_pairs, void *stream) {
    return group_clone_pairs(g, nullptr, pairs, n_pairs, stream, "reina_group_clone");
}

}  // extern "C"
