// sicp_batch.hip -- sicp_icp_run_batch (include/simpleicp_hip_batch.h): the chained ICP loops of many contexts behind one call.
//
// Each member is a ctx prepared as for sicp_icp_run.  A batched iteration is ONE match launch for every member (k_grid_nn_batch,
// sicp_grid.hip: k_grid_nn's body, a per-block member map) and one tail launch per k_icp_tail instantiation present
// (k_icp_tail_batch<EPT>, sicp_tail.hip: k_icp_tail's body, one workgroup per member).  Both read the member table this file builds
// in device memory; the loop state stays each member's own (IcpDev in its ctx), so a member's launches compute what its lone run's
// would, and its ctx ends in the state a lone run leaves.  Records stream into a pinned ring the first member's ctx owns, one
// REC_RING slice per member; the host reads them in launch order with the lone loop's own record handling (take_record).
#include "sicp_host.h"
#include "../../include/simpleicp_hip_batch.h"

#include <set>

namespace {

void set_status(sicp_batch_member &m, int rc)
{
    m.status = rc;
    if (rc == SICP_OK) m.error[0] = '\0';
    else std::snprintf(m.error, sizeof m.error, "%s", sicp_last_error());
}

// does the batched road compute exactly what sicp_icp_run would for this member?  (the one-wave-per-query grid search and the
// single-workgroup device tail: Q <= SOLVE_MAX_Q, the grid flavour, the device solver, no instrumentation)
bool batchable(sicp_ctx *c, const sicp_batch_member &m)
{
    if (check_iter_args(c, &m.params) != SICP_OK) return false;         // (joins the slots' background uploads: check_slot)
    if (!device_tail(c) || c->Q > SOLVE_MAX_Q || !takes_grid_search(c)) return false;
    if (normal_angle_on(c)) return false;                               // (its launches are not part of the batched chain)
    return !(c->timing || c->count_work || c->host_trace || c->solve_trace);
}

struct MemberRun {
    int64_t idx;                  // into the caller's list
    double xcur[6];
    double last_move;
    bool over;
};

}  // namespace

SICP_EXPORT int sicp_batch_version(void) { return SICP_BATCH_VERSION; }

SICP_EXPORT int sicp_ctx_lean(sicp_ctx *c)
{
    if (!c) return fail(SICP_ERR_INVALID, "null ctx");
    if (c->dl_shared) return SICP_OK;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->h_dl) { HIPCHK(hipHostFree(c->h_dl)); c->h_dl = nullptr; }     // (its own ring, if it had one: the shared one from now on)
    c->dl_shared = true;
    return SICP_OK;
}

SICP_EXPORT int sicp_icp_run_batch(sicp_batch_member *mem, int64_t count, int64_t *fallback_count)
{
    if (fallback_count) *fallback_count = 0;
    if (!mem || count <= 0) return fail(SICP_ERR_INVALID, "empty batch");
    // ---- batch-wide checks: nothing is launched, no member is touched ----
    std::set<sicp_ctx *> seen;
    for (int64_t i = 0; i < count; ++i) {
        sicp_ctx *c = mem[i].ctx;
        if (!c) return fail(SICP_ERR_INVALID, "member %lld: null ctx", (long long)i);
        if (!seen.insert(c).second) return fail(SICP_ERR_INVALID, "member %lld: its ctx is already in the batch", (long long)i);
        if (c->device != mem[0].ctx->device)
            return fail(SICP_ERR_INVALID, "member %lld: ctx on device %d, the batch runs on device %d", (long long)i, c->device, mem[0].ctx->device);
        if (c->Q <= 0) return fail(SICP_ERR_INVALID, "member %lld: call sicp_icp_setup first", (long long)i);
        if (c->collective())
            return fail(SICP_ERR_INVALID, "member %lld: an exchange or communicator is attached (multi-GPU runs are not batched)", (long long)i);
        if (mem[i].max_iterations > 0 && !mem[i].results) return fail(SICP_ERR_INVALID, "member %lld: null results", (long long)i);
    }
    sicp_ctx *c0 = mem[0].ctx;
    HIPCHK(hipSetDevice(c0->device));
    // ---- the batch's workspace, sized for every member being batched, BEFORE any member is touched: a failure here leaves them all
    //      as they were ----
    size_t map_cap = (size_t)count;
    for (int64_t i = 0; i < count; ++i) {
        map_cap += (size_t)((mem[i].ctx->Q + 3) / 4);
        if (!mem[i].ctx->batch_ev) HIPCHK(hipEventCreateWithFlags(&mem[i].ctx->batch_ev, hipEventDisableTiming));
    }
    if (c0->batch_ring_members < count) {
        if (c0->h_batch_ring) { (void)hipHostFree(c0->h_batch_ring); c0->h_batch_ring = nullptr; c0->batch_ring_members = 0; }
        const size_t bytes = (size_t)count * REC_RING * REC_DOUBLES * sizeof(double);
        HIPCHK(hipHostMalloc((void **)&c0->h_batch_ring, bytes, hipHostMallocMapped));
        std::memset(c0->h_batch_ring, 0, bytes);
        c0->batch_ring_members = (long)count;
    }
    CHK(c0->batch_tab.reserve((size_t)count));
    CHK(c0->batch_map.reserve(map_cap));
    std::vector<int64_t> fallback;
    std::vector<MemberRun> run;
    std::vector<BatchMember> tab;
    for (int64_t i = 0; i < count; ++i) {
        sicp_batch_member &m = mem[i];
        m.iterations = 0; m.path = SICP_BATCH_PATH_BATCHED;
        set_status(m, SICP_OK);
        if (m.max_iterations <= 0) continue;                             // (what sicp_icp_run does: nothing)
        sicp_ctx *c = m.ctx;
        if (!batchable(c, m)) { fallback.push_back(i); continue; }
        // a lone run's preparation, for this member on its own stream
        MemberRun r;
        bool grid;                                                       // (true: batchable)
        int rc = chain_prepare(c, &m.params, &grid, &r.last_move);
        if (rc == SICP_OK && hipEventRecord(c->batch_ev, c->stream) != hipSuccess) rc = fail(SICP_ERR_HIP, "hipEventRecord failed");
        if (rc != SICP_OK) { set_status(m, rc); continue; }
        const Cloud &cl = c->cloud[SICP_MOV];
        BatchMember e = {};
        e.st = c->icp_dev.p;
        e.qx = c->q.p; e.qy = c->q.p + c->qpad; e.qz = c->q.p + 2 * c->qpad;
        e.normals = c->normals.p; e.planarity = c->planarity.p;
        e.m_d2 = c->m_d2.p; e.m_idx = c->m_idx.p; e.m_p2 = c->m_p2.p;
        e.dist = c->dist.p; e.flag = c->flag.p; e.keep = c->keep.p; e.resid = c->resid.p;
        e.cell_start = cl.grid.cell_start.p; e.rec = cl.grid.rec.p; e.G = cl.grid.g;
        e.rmax = cl.rmax; e.idx_base = cl.idx_base;
        e.prev0 = c->have_prev_match ? c->m_p2.p : nullptr;
        e.A = tail_args(c, &m.params, run_min_change(m.min_change));
        e.max_it = m.max_iterations;
        tab.push_back(e);
        r.idx = i;
        std::memcpy(r.xcur, m.params.x, sizeof r.xcur);
        r.over = false;
        run.push_back(r);
    }
    const long B = (long)tab.size();
    if (B > 0) {
        // ---- the member table: block -> member map of the match launch, then the tail buckets' member lists ----
        std::vector<uint32_t> map;
        int depth = 1 << 30;
        int64_t max_all = 0;
        for (long k = 0; k < B; ++k) {
            const long blocks = ((long)tab[k].A.Q + 3) / 4;                // (4 waves per block, one query each)
            tab[k].blk0 = (uint32_t)map.size();
            map.insert(map.end(), (size_t)blocks, (uint32_t)k);
            depth = std::min(depth, mem[run[k].idx].ctx->chain_depth);
            max_all = std::max(max_all, tab[k].max_it);
        }
        const long nblk = (long)map.size();
        const int epts[4] = {1, 2, 4, 8};
        long b_off[4], b_cnt[4];
        for (int b = 0; b < 4; ++b) {
            b_off[b] = (long)map.size();
            for (long k = 0; k < B; ++k)
                if (icp_tail_ept(tab[k].A.Q) == epts[b]) map.push_back((uint32_t)k);
            b_cnt[b] = (long)map.size() - b_off[b];
        }
        for (long k = 0; k < B; ++k) tab[k].ring = c0->h_batch_ring + (size_t)k * REC_RING * REC_DOUBLES;
        const hipStream_t s0 = c0->stream;
        const int rc = [&]() -> int {
        // every member's preparation (grid, loop state) on its own stream comes first: the batch's stream waits for it on the device
        for (long k = 0; k < B; ++k) HIPCHK(hipStreamWaitEvent(s0, mem[run[k].idx].ctx->batch_ev, 0));
        HIPCHK(hipMemcpyAsync(c0->batch_tab.p, tab.data(), (size_t)B * sizeof(BatchMember), hipMemcpyHostToDevice, s0));
        HIPCHK(hipMemcpyAsync(c0->batch_map.p, map.data(), map.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s0));
        for (long k = 0; k < B; ++k) {
            sicp_ctx *c = mem[run[k].idx].ctx;
            c->have_prev_match = true;                                   // (as after a lone run's first launch)
            c->last_match_kernel = 2;
        }

        // ---- iterations back to back: `depth` launches ahead of the records being read ----
        double seqs[REC_RING];
        int64_t launched = 0, completed = 0;
        auto all_over = [&]() {
            for (long k = 0; k < B; ++k) if (!run[k].over && launched < tab[k].max_it) return false;
            return true;
        };
        while (true) {
            while (launched < max_all && launched - completed < depth && !all_over()) {
                const double seq = (double)(++c0->solve_seq);
                const int slot = (int)(launched % REC_RING);
                seqs[slot] = seq;
                launch_grid_nn_batch(s0, c0->batch_tab.p, c0->batch_map.p, nblk, launched);
                for (int b = 0; b < 4; ++b)
                    if (b_cnt[b] > 0) launch_icp_tail_batch(s0, epts[b], c0->batch_tab.p, c0->batch_map.p + b_off[b], b_cnt[b], launched, slot, seq);
                HIPCHK(hipGetLastError());
                ++launched;
            }
            if (completed == launched) break;
            const int slot = (int)(completed % REC_RING);
            for (long k = 0; k < B; ++k) {
                if (completed >= tab[k].max_it) continue;                // (launches past its limit left it alone: no record)
                const double *o = tab[k].ring + (size_t)slot * REC_DOUBLES;
                CHK(wait_ticket(c0, o + REC_TICKET, seqs[slot]));
                if ((int)o[REC_STATUS] == 3 || run[k].over) { run[k].over = true; continue; }   // launched after the end of its run
                sicp_batch_member &m = mem[run[k].idx];
                const int rc = take_record(m.ctx, &m.params, o, m.results, &m.iterations, run[k].xcur, &run[k].last_move, &run[k].over);
                if (rc != SICP_OK) set_status(m, rc);
            }
            ++completed;
        }
        // the last launches' loop-state stores land behind their records: every member's stream may use its ctx after this
        HIPCHK(hipStreamSynchronize(s0));
        return SICP_OK;
        }();
        if (rc != SICP_OK) {
            // a HIP failure of the batch itself: every member it held carries it (their contexts were touched)
            for (long k = 0; k < B; ++k) if (mem[run[k].idx].status == SICP_OK) set_status(mem[run[k].idx], rc);
            (void)hipStreamSynchronize(s0);
            return rc;
        }
    }
    // ---- members the batched kernels do not cover: their own sicp_icp_run ----
    for (int64_t i : fallback) {
        sicp_batch_member &m = mem[i];
        m.path = SICP_BATCH_PATH_FALLBACK;
        set_status(m, sicp_icp_run(m.ctx, &m.params, m.max_iterations, m.min_change, m.results, &m.iterations));
    }
    if (fallback_count) *fallback_count = (int64_t)fallback.size();
    return SICP_OK;
}
