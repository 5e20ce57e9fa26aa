// reina_hip.hip part: the clone of a logged group (include/reina_filter_log.h; DESIGN.md section 6d "Logged filters").
// Included behind k_filter.inc and k_course.inc: it uses the clone's pair list and geometry and the two logs' structs.
//
// ONE launch, k_txlog_clone, ahead of k_group_clone in every chunk of pairs: blockIdx.y = pair, blockIdx.x = four 512-agent
// tiles, one wave each.  A wave streams both members' hot words (k_group_clone's loop: lane l looks at agent 64 j + l of the
// tile in round j) and, where either is non-zero, copies the 4-byte log word and -- COURSE -- the 8-byte record from src to
// dst.  Agents susceptible in both members are not touched: by the logs' invariant (the header) their words are all NONE in
// both.  The hot words are only read: k_group_clone, queued behind on the same stream, moves them.  One lane owns an agent:
// plain stores, no atomics, no fences.
#include "../../include/reina_filter_log.h"

template <bool COURSE>
__global__ __launch_bounds__(CLONE_THREADS) void k_txlog_clone(const MemberRef *M_, uint32_t *log, crs_rec *rec, size_t stride, const ClonePairs a) {
    const uint32_t pr = a.p[blockIdx.y];
    const uint32_t dm = pr & 0xFFFFu, sm = pr >> 16;
    const uint32_t tile = blockIdx.x * CLONE_TILES_PER_BLOCK + (threadIdx.x >> 6);
    if (tile >= a.n_tiles) return;   // (whole waves)
    MemberRef dref, sref;
    member_from_constant(&dref, M_ + dm);
    member_from_constant(&sref, M_ + sm);
    const GAS uint32_t *dhot = (const GAS uint32_t *)dref.B.hot, *shot = (const GAS uint32_t *)sref.B.hot;
    GAS uint32_t *DL = (GAS uint32_t *)log + (size_t)dm * stride;
    const GAS uint32_t *SL = (const GAS uint32_t *)log + (size_t)sm * stride;
    GAS crs_rec *DC = (GAS crs_rec *)rec + (size_t)dm * stride;
    const GAS crs_rec *SC = (const GAS crs_rec *)rec + (size_t)sm * stride;
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll 4
    for (uint32_t j = 0; j < 8u; j++) {
        const uint32_t i = tile * 512u + j * 64u + lane;
        if (i >= a.n_agents) break;
        if ((shot[i] | dhot[i]) == 0u) continue;
        DL[i] = SL[i];
        if (COURSE) DC[i] = SC[i];
    }
}

// the log's launch of one chunk of pairs (group_clone_pairs, k_filter.inc)
static int txlog_clone_launch(reina_txlog *l, const MemberRef *d_refs, uint32_t tile_blocks, const ClonePairs &a, hipStream_t s) {
    if (l->course)
        hipLaunchKernelGGL(k_txlog_clone<true>, dim3(tile_blocks, a.n), dim3(CLONE_THREADS), 0, s, d_refs, l->d_log, l->course->d_rec, l->stride, a);
    else
        hipLaunchKernelGGL(k_txlog_clone<false>, dim3(tile_blocks, a.n), dim3(CLONE_THREADS), 0, s, d_refs, l->d_log, (crs_rec *)nullptr, l->stride, a);
    HIP_CHECK(hipGetLastError());
    return REINA_OK;
}

extern "C" {

int reina_filter_log_version(void) { return REINA_FILTER_LOG_VERSION; }

int reina_group_txlog_clone(reina_txlog_t *log, const uint32_t *pairs, uint32_t n_pairs, void *stream) {
    if (!log) return refuse("reina_group_txlog_clone: no log");
    if (int rc = attachment_kind(log, true, "reina_group_txlog_clone")) return rc;
    if (log->course && log->course->log != log) return refuse("reina_group_txlog_clone: the course is not attached to this log (its log is gone)");
    return group_clone_pairs(log->g, log, pairs, n_pairs, stream, "reina_group_txlog_clone");
}

}  // extern "C"
