// sicp_host.h -- what the host-side translation units of libsimpleicp_hip share: the context, the clouds and their grids, the error
// plumbing, and the internal functions that cross files.  sicp_api.cpp: context, errors, timing, small exports; sicp_clouds.cpp: uploads,
// downloads, grid builds; sicp_search.cpp: the 1-NN / k-NN drivers and their exports; sicp_icp.cpp: the iteration loop, the solvers,
// the operator-by-operator road; sicp_comm.cpp: RCCL loader, exchanges, communicator exports.
#ifndef SICP_HOST_H
#define SICP_HOST_H

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>          // types and prototypes only: librccl is loaded on demand (sicp_comm_init), never linked
#include <dlfcn.h>
#include <sched.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/simpleicp_hip.h"
#include "sicp_handover.h"
#include "sicp_internal.h"

using namespace sicp;

#define SICP_EXPORT extern "C" __attribute__((visibility("default")))

namespace sicph {

int fail(int code, const char *fmt, ...);

#define HIPCHK(expr)                                                                             \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return fail(SICP_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),     \
                        __FILE__, __LINE__);                                                     \
    } while (0)

#define CHK(expr)                  \
    do {                           \
        int rc_ = (expr);          \
        if (rc_ != SICP_OK) return rc_; \
    } while (0)

template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;   // elements
    int reserve(size_t n)
    {
        if (n <= cap) return SICP_OK;
        if (p) { HIPCHK(hipFree(p)); p = nullptr; cap = 0; }
        HIPCHK(hipMalloc((void **)&p, n * sizeof(T)));
        cap = n;
        return SICP_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

struct Grid {
    bool valid = false;
    GridGeom g;
    long ncells = 0;
    double avg_per_cell = 0;
    double target_used = 0;          // points per occupied cell the build aimed at (grid_build: rebuilt when the regime changes)
    bool cap_limited = false;        // the cell table's size limit, not the points-per-cell target, set the cell size
    double pointwise_occupancy = 0;  // sum c^2 / n over the cells: how many points share the cell of an average point
    bool nonuniform = false;         // the cell size was set by the points' own view (dense core), not by the average: wide balls cross
                                     // thousands of its rows -- such a cloud gets a coarse twin (Cloud::coarse_grid)
    DevBuf<uint32_t> cell_start;     // ncells + 1
    DevBuf<double> rec;              // the cloud in cell order: packed 32-byte records (x, y, z, local row as int64 bits)
    // companions, built the first time a search wants them (grid_companions) and dropped with the grid:
    DevBuf<float> recf;              // the cloud in cell order as 16-byte float32 records relative to c0 (the filtered many-queries search)
    DevBuf<unsigned long long> cell_box;   // the cells' tight boxes + counts (far searches trim their rows by them)
    bool recf_valid = false, box_valid = false;
    double c0[3] = {0, 0, 0}, eps_p = 0;   // float32 frame: centre of the cloud's box; 6e-8 x the largest |coordinate - c0|
    bool filter_ok = false;          // float32 can hold the cloud (half extents below 1e15)
};

struct Cloud {
    int64_t n = 0, npad = 0, idx_base = 0;
    double rmax = 0.0;    // largest point norm (error bounds of the filtered / grid searches)
    double bb_lo[3] = {0, 0, 0}, bb_hi[3] = {0, 0, 0};   // bounding box (measured with rmax in the upload's one statistics pass)
    Grid grid;
    DevBuf<float> pl;     // `planarity` column by GLOBAL index (pl_n entries; 0 = the cloud has no such column)
    int64_t pl_n = 0;
    DevBuf<double> xyz;   // x[npad] | y[npad] | z[npad]
    // rejection by the angle between normals (sicp_nangle.hip): the cloud's own normal columns by GLOBAL index (nv_n points; 0 = none),
    // else normals estimated on demand, kept by local index with one "is there" bit per point (a normal that is there may be NaN)
    DevBuf<float> nv; int64_t nv_n = 0;
    DevBuf<float> nrm2; DevBuf<uint32_t> nrm2_have;
    bool nrm2_valid = false; int nrm2_k = 0;       // (emptied where the grid is invalidated: another cloud, a transform; or another k)
    // every 64th point with a grid of its own (built on demand for a cold chained search): the nearest SUBSAMPLE point is a cloud
    // point, so its distance bounds the answer -- one cheap search hands the real one a radius instead of a doubling ladder
    DevBuf<double> sub_xyz; int64_t sub_n = 0, sub_npad = 0;
    Grid sub_grid;
    Grid coarse_grid;     // ALL points again in cells 8 x as wide, only for clouds whose grid is `nonuniform`: the exact search's wide passes
    const double *x() const { return xyz.p; }
    const double *y() const { return xyz.p + npad; }
    const double *z() const { return xyz.p + 2 * npad; }
    double *x() { return xyz.p; }
    double *y() { return xyz.p + npad; }
    double *z() { return xyz.p + 2 * npad; }
};

// RCCL entry points, resolved the first time a communicator is asked for (single-GPU users never load the library)
struct Rccl {
    void *h = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    decltype(&ncclCommCount) CommCount = nullptr;
    decltype(&ncclCommUserRank) CommUserRank = nullptr;
    decltype(&ncclCommAbort) CommAbort = nullptr;
    std::string why;               // why the library is unusable (dlerror is read ONCE, where it is fresh)
};

// rejection by the angle between normals: the ctx's setting and the buffers of an iteration's launches (sicp_nangle.hip)
struct NormalAngle {
    double cos_max = 0.0;          // > 0: sicp_icp_run / sicp_icp_iterate reject by contract (N)
    int k = 0;                     // neighbours of the normals estimated on demand
    int par = 0;                   // which counter pair the next iteration's launches use
    long iota_n = 0;               // leading words of `iota` that hold 0, 1, 2, ... (0: the four-per-wave sweep's spill list was written there)
    bool counters_stale = false;   // sicp_icp_setup since the counters were last cleared
    DevBuf<unsigned> cnt;          // sicp_nangle.hip: NA_*
    DevBuf<uint32_t> list_q, list_m, iota;   // the miss list (correspondence, local point); 0, 1, 2, ... or the sweep's spill list
    DevBuf<double> cov;            // (list position, 6)
    DevBuf<float> per_q;           // the operator's per-correspondence normals
};

struct EventPair { hipEvent_t a, b; int kernel; };
constexpr int REC_RING = 16;     // records in flight + being read
static_assert(REC_RING == HANDOVER_RING, "sicp_handover.h indexes the same ring");

inline long round_up(long v, long g) { return (v + g - 1) / g * g; }
inline double wall_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
inline bool is_observed(double w) { return w > 0 && std::isfinite(w); }
inline void H16_to_Xf(const double H[16], Xf *o) { for (int i = 0; i < 12; ++i) o->m[i] = H[i]; }

}  // namespace sicph
using namespace sicph;

// an upload running behind its caller (sicp_cloud_upload_start): the helper thread and what it left
struct BgUpload {
    std::thread th;
    bool active = false;
    int rc = SICP_OK;
    std::string err;
};

struct sicp_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr;   // background uploads: their DMA, layout kernel and statistics pass
    BgUpload bg[2];                // by slot; at most one is active
    DevBuf<double> stage_bg;       // ... their AoS staging block
    DevBuf<double> bg_small;       // ... their statistics scratch (7 words) and its pinned mirror
    double *h_bg = nullptr;
    hipDeviceProp_t prop;
    Cloud cloud[2];
    DevBuf<double> stage;          // AoS staging for uploads / downloads / query sets
    // scan workspace
    DevBuf<double> part_d2;
    DevBuf<uint32_t> part_idx;
    DevBuf<double> kq;             // SoA queries of sicp_knn: qx|qy|qz
    DevBuf<double> k_d2;           // (Q,k) results
    DevBuf<int64_t> k_idx;
    DevBuf<double> floor_d2;
    DevBuf<uint32_t> floor_idx;
    DevBuf<double> bound;          // per-query upper bound of the NN distance (filtered scan)
    DevBuf<double> x_send, x_recv; // exchange records: [Q][5] and [world][Q][5]
    int fs_blocks_per_cu[2] = {0, 0};   // occupancy of k_knn1_fscan<128>, <256>
    int fr_blocks_per_cu[2] = {0, 0};   // occupancy of k_knn1_frec<128>, <256>
    int fscan_variant = 0;         // SICP_FSCAN = record (default: VALU filter, candidates recorded) | inline
    long fscan_cap = 0;            // SICP_FSCAN_CAP: recorded groups per query (tests force overflow with tiny values)
    DevBuf<uint32_t> hit_cnt, hit_list;
    int knn1_mode = 0;             // SICP_KNN1 = exact | filter | grid: force one 1-NN flavour (A/B + tests); 0 = auto
    DevBuf<uint32_t> g_ids, g_counts, g_cursor, g_blk;    // grid build scratch: cell ids, histogram, scatter cursors, scan partials
    DevBuf<unsigned long long> match_work;                // [0] candidates evaluated, [1] grid rows visited, [2] launches (instrumented runs); [4..7] the k-NN sweep's tallies
    DevBuf<unsigned long long> rj_keys;   // large-Q rejection scratch: Q keys + the selection state
    bool have_prev_match = false;  // m_p2 holds last iteration's winners (bound source)
    DevBuf<uint32_t> q_order;      // large query sets: the queries [q_order_lo, +q_order_cnt) in cell order (search locality)
    long q_order_lo = -1, q_order_cnt = 0;
    long order_min_q = 32768;      // SICP_ORDER_MIN_Q: from this many queries per launch on (0: never)
    DevBuf<uint32_t> k_order;      // the queries of a k-NN / normals call in cell order
    DevBuf<int64_t> k_sel;         // sicp_estimate_normals: selected rows, normals and planarity before they leave
    DevBuf<float> k_nv, k_pl;
    DevBuf<double> k_cov;          // (Q, 6) covariances between the k-NN sweep and the eigen step
    DevBuf<uint32_t> k_redo;       // [0] count, [1..] slots the four-queries-per-wave sweep left to the one-query-per-wave kernel
    int knn_group = 0;             // SICP_KNN_GROUP = 1 / 4: queries per wave of the k-NN sweep (0: chosen per launch)
    long knn_batch = 0;            // SICP_KNN_BATCH: queries a wave of the one-sweep k-NN works through (0: chosen per launch)
    bool knn_sweep = true;         // SICP_KNN_SWEEP=0: k extraction rounds (k_grid_knn) + k_normals instead of the one-sweep kernel
    DevBuf<double> bound_p2, bound_d2;   // cold search: nearest subsample point per query (coordinates = the bound) + scratch
    DevBuf<int64_t> bound_idx;
    int coarse_iters = 1;          // chained iterations (from a cold start) whose search is bounded by the subsample's (more than one helped nowhere)
    long coarse_min_n = 262144;    // ... for clouds of at least this many points
    long nn16_min_q = 5120;        // SICP_NN16_MIN_Q: from this many queries per launch on the grid search runs four queries per wave.  Round 5 measured
                                   // the crossover at 8 192 -- when the four-per-wave kernel still needed k_postmatch's launch behind it; with its own
                                   // distance epilogue (round 6, below 65 536 queries) it wins from ~5 000: match per launch at 4 096 / 6 000 / 8 191
                                   // queries 13.4 / 16.0 / 19.2 us with one wave per query, 15.3 / 14.5 / 15.6 with four (profiles/r6/nn16_crossover.txt)
    int nn16_filter = 2;           // SICP_NN16 = exact (0: k_grid_nn16) | far (1: the filtered search, one flavour) | near (2, default: the lean
                                   // flavour first, the full one for what it leaves)
    int dl_threads = 16;                  // host threads of sicp_cloud_download_both: one feeds the link, the others fan the chunks out into the caller's arrays
                                          // (round 6: with 15 of them the call waits 4.8 of its 5.3 ms for the link -- profiles/r6/download_parts_ring_packed_streamed.txt)
    int grid_cap_nonuniform_log2 = 27;    // log2 of the cell table's limit for clouds whose points crowd a few cells
    bool grid_pointwise = true;    // the cell size follows the POINT-weighted occupancy (false: the average over occupied cells only -- round 4's rule)
    long nn16f_min_q = 196608;     // SICP_NN16F_MIN_Q: from this many queries per launch on the many-queries search goes through the float32 filter
    bool nn16f_min_q_forced = false;   // (the environment named it: no per-cloud adjustment)
                                   // (below: its two extra launches cost more than the filter saves on a machine that is not full)
    double far_move = 0.75;        // SICP_FAR_MOVE: the lean flavour goes first once the estimate moves by less than this many cells per iteration
    bool dl_shared = false;        // sicp_ctx_lean: h_dl is the ring the process's lean contexts share (sicp_clouds.cpp: dl_ring), not this ctx's
    bool upload_staged = true;     // small uploads go through the pinned buffer (false: every upload a DMA straight out of the caller's arrays)
    bool use_boxes = false;        // SICP_BOXES=1: far searches trim their rows by the cells' tight boxes.  OFF by default: measured (profiles/r5), the
                                   // boxes cut 14-30 % of the candidates and never a microsecond -- DESIGN.md section 4
    bool boxes_always = false;     // SICP_BOXES=2: ... and stand-alone searches of a handful of queries build them too (tests)
    DevBuf<double> q_slot, p_slot; // filtered search: queries (x, y, z, index) and their last matches in SLOT order (32 bytes each)
    long slot_lo = -1, slot_cnt = 0;
    bool slot_ordered = false;
    DevBuf<double> kq_slot, kp_slot;   // ... of a stand-alone search (sicp_knn k = 1, sicp_select_in_range, the operators): the run's stay untouched
    DevBuf<uint8_t> nn_state;      // by slot: 1 = the lean flavour left this query to the full one
    DevBuf<uint32_t> nn_redo;      // [0], [1] counters (alternating by launch), [2..] queries left to the exact kernel
    int nn_parity = 0;
    double last_move = 0.0;        // displacement at the cloud's edge the last completed iteration caused (far / lean flavour choice)
    int last_match_kernel = 0;     // 0 exact scan, 1 filtered scan (inline), 2 grid, 3 filtered scan (record + fix-up), 5 grid, four queries per wave (exact), 6 grid, float32 filter
    // ICP state (selected fixed points and per-iteration products)
    int64_t Q = 0, qpad = 0;
    DevBuf<double> q;              // qx|qy|qz [qpad]
    DevBuf<float> normals, planarity;
    DevBuf<int64_t> m_idx;         // matched movable index (global)
    DevBuf<double> m_d2, m_p2, dist, resid;
    DevBuf<uint8_t> flag, keep;
    DevBuf<double> small;          // [0..3] reject out, [4..6] stats out, [8..37] normal equations
    DevBuf<double> ne_partial;
    DevBuf<unsigned> ticket;
    double *h_small = nullptr;     // pinned mirror of `small`
    double *h_dl = nullptr;        // pinned buffers of sicp_cloud_download_both (a ring of 4 x 3 x 256 Ki doubles) and of the staged uploads (2 x 3 x 512 Ki), on first use
    hipEvent_t dl_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool have_iter = false;
    bool have_corr = false;        // sicp_corr_match has run: m_idx / m_p2 / dist hold its correspondences, `keep` the alive mask
    NormalAngle na;
    DevBuf<float> corr_pl;         // per-correspondence planarity columns handed to sicp_corr_reject_planarity: pc1 [Q] | pc2 [Q]
    double last_x[6] = {0}, last_w = 1.0, last_obs[6] = {0}, last_ow[6] = {0};
    double last_ne[30] = {0};      // normal equations at last_x (fused path caches them)
    double last_tail_cycles[5] = {0};   // k_icp_tail's own clock over its phases, last iteration (sicp_tail_cycles)
    long last_sel_rounds[2] = {0, 0}, sel_window_hits = 0;   // ... how it found median / MAD (sicp_tail_selection)
    bool have_last_ne = false;
    int solve_mode = 0;            // SICP_SOLVE = fused | host (A/B + tests); 0 = auto
    bool grid_target_forced = false;   // (kept for a caller that pins the target: every grid uses it then)
    double grid_target = 16.0;     // points per occupied grid cell the cell size aims at (
                                   // measured flat from 12 to 32, 5-20 % slower below 8: fewer, longer rows win)
    bool host_trace = false;       // SICP_SOLVE_TRACE=host: per-iteration host timings on stderr
    bool solve_trace = false;      // SICP_SOLVE_TRACE: the fused kernel's cycle counters on stderr
    bool trace_sel = false, trace_eval = false;   // SICP_SOLVE_TRACE=sel / eval: the fine splits of a trace build
    long solve_seq = 0;            // completion tickets of the fused kernel
    DevBuf<IcpDev> icp_dev;        // device-resident loop state of a chained run (sicp_tail.hip)
    DevBuf<LmDev> lm_dev;          // solver state of the multi-workgroup evaluation chain (sicp_lm.hip)
    LmDev *h_lm = nullptr;         // pinned staging of it
    DevBuf<double> resid2;         // second residual buffer of that chain (trial / accepted alternate)
    int resid_slot = 0;            // which buffer holds the last iteration's accepted residuals
    int lm_evals = 4;              // evaluations enqueued per iteration for Q > SOLVE_MAX_Q (k_lm_finish completes the rest)
    double *h_rec = nullptr;       // pinned ring of per-iteration records the tail kernel streams to the host
    IcpDev *h_state = nullptr;     // pinned staging of the loop state
    DevBuf<unsigned long long> lm_bar_buf;   // grid barrier of the one-launch minimisation (zeroed when allocated)
    unsigned long long lm_bar = 0;     // what its launches have added to the counter so far
    bool lm_one_launch = true;         // SICP_LM=launches: one launch per evaluation + finish (A/B; always with a sharded reduction)
    unsigned long long hsel_bar = 0;   // what the one-launch rejection's launches have added to its barrier counter so far
    int test_barrier_fault = 0;    // SICP_TEST_BARRIER_FAULT = 1 / 2 (tests only): the rejection's / the solver's grid barrier expects a block that never comes
    bool tail_window = true;       // SICP_TAIL_WINDOW=0: the single-workgroup tail never looks for median / MAD in a window around the last iteration's (A/B, tests)
    bool reject_prior = false;     // c->small[0..3] holds the last chained k_reject launch's statistics for the current setup
    bool hsel_window = true;       // SICP_HSEL_WINDOW=0: never the windowed (three-barrier) form of the large-Q rejection
    long hsel_run_launches = 0;    // chained rejection launches since the last setup (the window needs two of them behind it)
    bool hsel_dirty = false;
    int nn_group = 0;              // SICP_NN_GROUP=8|16: lanes per query of the many-queries search (0: chosen per launch)
    // the tail -> match hand-over of a small-Q chain: iterations alternate between `stream` and `stream2`, the match of
    // iteration i + 1 is launched early and waits for the ticket tail i publishes in pre_tkt (PRE_TKT_WORDS words, zeroed at creation)
    hipStream_t stream2 = nullptr;
    hipEvent_t pre_ev = nullptr;       // a run's setup + first match are enqueued on `stream`: stream2 waits for it once per run
    DevBuf<unsigned long long> pre_tkt;
    bool chain_prelaunch = true;       // SICP_CHAIN_PRELAUNCH=0: the single-stream chain (A/B, tests)
    bool pre_running = false;          // a run that hands over early is between its first launch and its last record: wait_ticket's slow path waits for both streams
    int64_t pre_last_run = 0, pre_total = 0;   // matches launched early in the last chained run / since the context was created
    int chain_depth = 4;           // iterations enqueued ahead of the last record read (two are not enough, four are: profiles/r2/ab_chain_depth.txt)
    // sicp_icp_run_batch with this ctx as its FIRST member (sicp_batch.hip): the member table, the match's block -> member map followed
    // by the tail buckets' member lists, and the pinned ring the members' records land in (B x REC_RING x REC_DOUBLES); grown, never shrunk
    DevBuf<BatchMember> batch_tab;
    DevBuf<uint32_t> batch_map;
    double *h_batch_ring = nullptr;
    long batch_ring_members = 0;
    hipEvent_t batch_ev = nullptr;   // ... a member's preparation done on its own stream (the batch's stream waits for it)
    // sicp_select_n_device (sicp_device.hip): per-block counts | their offsets | the total (4 bytes per 1 024 points), the Q picked
    // positions (the kept rows themselves are stream-ordered memory of the call)
    DevBuf<uint32_t> sel_blk;
    DevBuf<int64_t> sel_pos;
    // a whole-cloud operator call's candidates (take_candidates): their rows, the verdict bytes on their way out; and the counter
    // words of every stand-alone operator (counters_clear / counters_fetch / counters_host below)
    DevBuf<int64_t> cand_rows;
    DevBuf<uint8_t> cand_keep;
    DevBuf<unsigned long long> cand_small;
    // voxel selection (sicp_voxel.hip): the hash table of {key, winner} word pairs, every candidate's slot in it (the first counter
    // word as two 32-bit ones: the kept count, the error bits)
    DevBuf<unsigned long long> vx_tab;
    DevBuf<uint32_t> vx_slot;
    // sicp_evaluate (sicp_eval.hip): the workgroups' partial sums and the levels above them, their inlier counts, the record on its
    // way out; grown, never shrunk, gone with the ctx
    DevBuf<double> ev_part, ev_out;
    DevBuf<long long> ev_cnt;
    // outlier filters (sicp_outlier.hip): d_i per position, the staged counts, the trees' partials (counter words: OL_*)
    DevBuf<double> ol_d, ol_part;
    DevBuf<uint32_t> ol_cnt;
    long outlier_chunk = 0;        // SICP_OUTLIER_CHUNK: candidates per search of the outlier filters (0: chosen per call; what a chunk holds is (chunk, k) distances)
    // FPFH descriptors (sicp_fpfh.hip): the normals as they are used (oriented), the counts of pass 1 ((n, 34) uint16), the staging
    // buffer of the descriptors
    DevBuf<float> fp_nrm, fp_out;
    DevBuf<uint16_t> fp_cnt;
    long fpfh_chunk = 0;           // SICP_FPFH_CHUNK: points per search of sicp_fpfh (0: chosen per call)
    // ISS keypoints (sicp_keypoints.hip): the saliency of pass 1 by point (the salient rows lie in cand_rows, the verdict bytes on
    // their way out in cand_keep), the staging buffers of the eigenvalues
    DevBuf<double> kp_sal, kp_eig;
    long keypoint_chunk = 0;       // SICP_KEYPOINT_CHUNK: points per search of sicp_keypoints (0: chosen per call)
    // DBSCAN labels (sicp_cluster.hip): the union-find's parent words, every point's root (0xffffffff: none), the roots' ranks
    // followed by the scan's block sums, the clusters' sizes, the staged labels (the core bytes are staged in cand_keep, the capped
    // counts land in ol_cnt)
    DevBuf<uint32_t> cl_parent, cl_root, cl_rank, cl_size;
    DevBuf<int32_t> cl_labels;
    long cluster_chunk = 1L << 22; // SICP_CLUSTER_CHUNK: points per launch of sicp_cluster's ball walks
    // planes of a cloud (sicp_plane.hip): the hypotheses' planes where the caller takes none, the refitted planes' states between
    // the launches, the staged mask and keep bytes (the rows are staged in gl_src, the triples in gl_tri, the planes that come in
    // in pf_in, the outputs in gl_pose / gl_idx; the spans' partial sums and counts lie in pf_part / pf_part2 / pf_cnt)
    DevBuf<double> pl_plane, pl_state;
    DevBuf<uint8_t> pl_mask, pl_keep;
    long plane_span = 0;           // SICP_PLANE_SPAN: rows a workgroup of sicp_plane_triplets' scoring kernel takes (0: chosen per call)
    // farthest point sampling (sicp_farthest.hip): every row's m_i and the workgroups' partial maxima of both parities (the stepped
    // path), the staged mask, picks and distances (the rows are staged in gl_src)
    DevBuf<double> fp_m, fp_part, fp_d2;
    DevBuf<uint8_t> fp_mask;
    DevBuf<int64_t> fp_idx;
    long farthest_one_max = 12288; // SICP_FARTHEST_ONE_MAX: the largest n on the single-workgroup path, at most SICP_FARTHEST_ONE_LIMIT (0: never).
                                   // The default is that limit: measured, 1 024 picks take 1.5 - 2.8 ms there at every n up to it and 3.9 - 4.3 ms
                                   // stepped, which is its launches (profiles/farthest/)
    long farthest_span = 0;        // SICP_FARTHEST_SPAN: rows a workgroup of the stepped path takes, whole waves of 64 (0: chosen per call)
    // consistent normal orientation (sicp_orient.hip): the k-NN lists as an (k, n) table, the normals as they came, the staging
    // buffers of the outputs, every point's root and sign, the union words of the roots, a component's offers (8 bytes of c, 8 of
    // the edge; behind the rounds its votes and its anchor)
    DevBuf<int32_t> or_nbr;
    DevBuf<float> or_nrm, or_out;
    DevBuf<uint32_t> or_comp, or_par;
    DevBuf<unsigned long long> or_bestc, or_beste;
    DevBuf<uint8_t> or_flip;
    long orient_chunk = 0;         // SICP_ORIENT_CHUNK: points per search of sicp_orient (0: chosen per call)
    // smooth regions (sicp_regions.hip) own no buffer: the lists lie in or_nbr, the staged normals in or_nrm, the staged seed bytes
    // in or_flip, every point's kind byte in cand_keep, and the union, root, rank (+ block sums), size and label words in the cl_ buffers
    long regions_chunk = 0;        // SICP_REGIONS_CHUNK: points per search of sicp_regions (0: chosen per call)
    // moving-least-squares smoothing (sicp_denoise.hip) owns no buffer either: host outputs are staged in kp_eig (the points), or_out
    // (the normals) and kp_sal (the displacements)
    long denoise_chunk = 0;        // SICP_DENOISE_CHUNK: points per search of sicp_denoise (0: chosen per call)
    // descriptor matching and RANSAC poses (sicp_global.hip): the queries' keys (bits(d2) << 32 | row) and the staging buffers of
    // the call's arrays
    DevBuf<unsigned long long> gl_key;
    DevBuf<float> gl_q, gl_t, gl_d2;
    DevBuf<int32_t> gl_idx, gl_tri;
    DevBuf<double> gl_src, gl_dst, gl_pose;
    long match_chunk = 0;          // SICP_MATCH_CHUNK: target rows per chunk of sicp_feature_match (0: chosen per call)
    // least-squares poses (sicp_posefit.hip): the staged input poses, the poses' states between the launches, the spans' partial
    // sums and the level above them, the spans' inlier counts (src, dst and the outputs are staged in the gl_ buffers)
    DevBuf<double> pf_in, pf_state, pf_part, pf_part2;
    DevBuf<uint32_t> pf_cnt;
    // robust poses (sicp_robust.hip): the poses' states between the launches of the sweeps path, the staged scales (the partial
    // sums lie in pf_part / pf_part2, the other arrays are staged where sicp_posefit.hip stages them)
    DevBuf<double> rb_state, rb_scale;
    int robust_path = 0;           // SICP_ROBUST: 1 "sweeps", 2 "one" -- the path of sicp_pose_robust where both apply (0: chosen per call)
    // length consistency of matches (sicp_consistency.hip): the compatibility matrix as bits (m rows of ceil(m / 64) words), the
    // peeling's remaining degrees, frontier bits and level words, the staged core numbers (src and dst are staged in gl_src / gl_dst,
    // the degrees in gl_idx)
    DevBuf<unsigned long long> cs_bits, cs_front;
    DevBuf<int32_t> cs_work, cs_core;
    DevBuf<unsigned> cs_state;
    int consistency_path = 0;      // SICP_CONSISTENCY: 1 "sweeps", 2 "one" -- the peeling of sicp_match_consistency where both apply (0: chosen per call)
    // exchange: an RCCL communicator of the library's own (sicp_comm_init) or a host callback (sicp_set_exchange)
    sicp_exchange_fn xfn = nullptr;
    void *xuser = nullptr;
    int last_xchg_form = 0; long xchg_count = 0;   // sicp_exchange_info: 1 records all-gather, 2 key all-reduces, 3 query slices
    bool xfn_u64 = false;          // the callback serves SICP_XCHG_MIN_U64 / MAX_U64 (asked once, at registration)
    ncclComm_t comm = nullptr;
    bool comm_active = false;      // a communicator stays with the ctx between runs (sicp_comm_activate): building one costs ~0.1-1 s
    int comm_rank = 0, comm_world = 1;
    long xkeys_min_q = 32768;      // SICP_XCHG_KEYS_MIN_Q: cloud shards from this many queries on exchange their winners by three all-reduces on
                                   // 8-byte keys instead of an all-gather of 40-byte records (0: never; the library's own communicator only)
    double xchg_timeout_s = 120.0; // a record that does not arrive within this while collectives are in flight = SICP_ERR_EXCHANGE, not a hang
    DevBuf<double> lm_gsum;        // sharded 6x6 reduction on the device solver: this rank's 8x8 Gram block, summed over ranks in place
    bool resid_sharded = false;    // ... after which only this rank's slice of the residuals is current (recomputed on demand)
    int rank = 0, world = 1, gn_shard = 0;
    int partition = SICP_PART_CLOUD;   // what is sharded over the ranks: the searched cloud or the queries
    bool collective() const { return xfn != nullptr || (comm != nullptr && comm_active); }
    // timing
    bool timing = false;
    bool count_work = false;       // sicp_timing_enable(ctx, 2): the grid search also tallies its candidates / rows
    std::vector<EventPair> pending, pool;
    double t_ms[SICP_K_COUNT] = {0};
    int64_t t_n[SICP_K_COUNT] = {0};
};

// from how many queries per launch the float32 filter takes a cloud's searches: a nonuniform cloud's alternative is one wave per query
// (the terrestrial stand-in at 100 000 queries: 0.60 ms per match against 0.53 through the filter), a uniform cloud's the four-per-wave kernel
inline long filter_min_q(const sicp_ctx *c, bool nonuniform)
{
    return (nonuniform && !c->nn16f_min_q_forced && c->nn16f_min_q > 65536) ? 65536 : c->nn16f_min_q;
}
// does a chained run match by the pruned exact search on the static grid?  (it serves every rigid H, i.e. every H(x) of the loop)
inline bool takes_grid_search(const sicp_ctx *c) { return (c->knn1_mode == 0 || c->knn1_mode == 3) && c->cloud[SICP_MOV].n < (1LL << 31); }
// sicp_icp_run's convergence threshold as the device tail takes it (negative there means "no test": the single-iteration API's)
inline double run_min_change(double min_change) { return std::isnan(min_change) || min_change < 0 ? 0.0 : min_change; }
// does a search of n queries on this grid ask for the float32 filter (sicp_gridf.hip)?  (whether float32 can hold the cloud is known
// once its companions are built: Grid::filter_ok)
inline bool wants_filter(const sicp_ctx *c, const Grid &gr, long n)
{
    return n > 0 && n >= c->nn16_min_q && n >= filter_min_q(c, gr.nonuniform) && c->nn16_filter != 0;
}
// a GridSearch's level: this grid, with its float32 companion
inline void set_level(GridSearch &S, const Grid &gr)
{
    S.G = gr.g; S.cell_start = gr.cell_start.p; S.rec = gr.rec.p; S.recf = gr.recf.p; S.c0 = gr.c0; S.eps_p = gr.eps_p;
}
// the search S on the cloud's subsample instead, for any of its points near the query (NN_APPROX): a bound for the search proper
inline GridSearch bound_search(GridSearch S, const Grid &sub, double *d2, int64_t *idx, double *p2)
{
    set_level(S, sub);
    S.coarse = nullptr; S.cell_box = nullptr; S.idx_base = 0; S.d2 = d2; S.idx = idx; S.p2 = p2; S.work = nullptr; S.flags = NN_APPROX;
    return S;
}
namespace sicph {

// The filtered many-queries search (sicp_gridf.hip) of S.Q queries, ties and all: see filtered_search (sicp_search.cpp).  What its two
// users -- a stand-alone search, a chained iteration's match -- do differently is named here and decided by them.
struct FilteredSearch {
    GridSearch S;                  // by-query columns, the level (set_level), coarse twin / boxes, transform, outputs, work;
                                   // S.prev_p2 + redo_flags: what bounds the exact redo of the ties
    DevBuf<double> *q_slot, *p_slot;   // the slot-ordered copies of the queries and their bounds: the run's own or a stand-alone search's
    bool fill_slots;               // ... are (re)written first, in S.order, bounds from slot_prev (null: none)
    const double *slot_prev;
    const Grid *cold;              // nullable: the subsample's grid -- a cold pre-pass leaves its nearest point in the slots as the bound
    int lanes;                     // lanes per query: 16 or 8
    bool all_far;                  // no lean flavour first: the full one takes all slots
    int redo_flags;
};
int filtered_search(sicp_ctx *c, const FilteredSearch &F);

// The ball operators' host side (sicp_outlier.hip; the radius filter and sicp_cluster.hip walk the same balls with the kernels of
// sicp_ball_dev.h).  ball_level: the grid level a ball of `radius` is walked on -- the slot's own grid, built if there is none --,
// refused with the radius filter's message where the ball's box of cells exceeds SICP_OUTLIER_MAX_BOX_CELLS.
int ball_level(sicp_ctx *c, int slot, double radius, GridLevel *lv);
// A walk over n rows of the slot, `chunk` of them per launch: enter(lo, cnt) gathers rows d_rows[lo, lo + cnt) (null: rows lo, lo + 1,
// ...) as columns in c->kq, qpad apart, and from SICP_ORDER_MIN_Q rows on builds their cell order (cells of twice the level's size,
// at most 1 << 22 of them); a job that fits one chunk keeps both for the walks that follow.  reserve(): c->kq for the largest chunk.
// grid(cnt): a ball kernel's workgroups over the chunk -- the one place that knows the groups per block and the round-up to 8 blocks.
struct BallChunks {
    sicp_ctx *c; int slot; const GridLevel &lv; const int64_t *d_rows; long n, chunk;
    bool kept = false;
    long qpad = 0;
    const uint32_t *order = nullptr;
    int reserve();
    int enter(long lo, long cnt);
    unsigned grid(long cnt) const;
    const double *qx() const { return c->kq.p; }
    const double *qy() const { return c->kq.p + qpad; }
    const double *qz() const { return c->kq.p + 2 * qpad; }
};
// k_ball_count enqueued over the cnt candidates of the chunk W stands in: keep = count >= cap, cnt_out = min(count, cap) (at pos[q],
// null: at q), *kept_total += the kept (null: not counted)
int ball_count_enqueue(const BallChunks &W, const int64_t *pos, long cnt, double radius, unsigned cap, uint8_t *keep, uint32_t *cnt_out,
                       unsigned long long *kept_total);

struct Timed {
    sicp_ctx *c; EventPair ev; bool on;
    Timed(sicp_ctx *ctx, int kernel) : c(ctx), on(ctx->timing)
    {
        if (!on) return;
        if (!c->pool.empty()) { ev = c->pool.back(); c->pool.pop_back(); }
        else {
            // timing-only events: no system-scope fence (cache write-back + invalidate) at every record --
            // the default flavour cost 13 us per ICP iteration on the stream it was measuring
            (void)hipEventCreateWithFlags(&ev.a, hipEventDisableSystemFence);
            (void)hipEventCreateWithFlags(&ev.b, hipEventDisableSystemFence);
        }
        ev.kernel = kernel;
        (void)hipEventRecord(ev.a, c->stream);
    }
    ~Timed()
    {
        if (!on) return;
        (void)hipEventRecord(ev.b, c->stream);
        c->pending.push_back(ev);
    }
};


Rccl *rccl();
void euler_R(const double a[3], double R[9]);
void euler_dR(const double a[3], double dR[27]);
void params_to_H12(const double x[6], double H12[12]);
bool spd_solve(int m, double *A, double *b);
int sync(sicp_ctx *c);
void collect_ready(sicp_ctx *c);
void abandon_exchange(sicp_ctx *c);
int wait_ticket(sicp_ctx *c, const double *flag_word, double seq);
int all_gather_f64(sicp_ctx *c, double *send, double *recv, long count);
int all_reduce_sum_f64(sicp_ctx *c, double *buf, long count);
int exchange_best(sicp_ctx *c, double *d2, int64_t *idx, double *p2, long Q);
int exchange_best_chained(sicp_ctx *c, const TailArgs &A, long Q, bool packed_by_match);
bool exchange_by_keys(const sicp_ctx *c, long Q);
int exchange_best_keys_chained(sicp_ctx *c, const TailArgs &A, long Q);
int all_reduce_u64(sicp_ctx *c, unsigned long long *buf, long count, bool take_max);
long query_slice(const sicp_ctx *c, long Q, long *lo);
int exchange_query_slices_idx(sicp_ctx *c, const TailArgs &A, long Q, bool packed_by_match);
void plan_chunks(const sicp_ctx *c, long npad, long qblocks, size_t bytes_per_chunk_row, int *chunk_pts, int *nchunks);
int reject_select(sicp_ctx *c, long Q, double *host_out, double seq, const IcpDev *st);
int reset_barrier_state(sicp_ctx *c);
int barrier_timed_out(sicp_ctx *c);
int check_slot(sicp_ctx *c, int slot, bool need_data);
int check_rows(const int64_t *rows, int64_t m, int64_t n, const char *what);
int check_candidate_rows(const int64_t *rows, int64_t m, int64_t n);
int check_device_ptr(sicp_ctx *c, const void *p, const char *what);
// is p memory of the ctx's device?  (a kernel may read and write it then; anything else goes through a staging buffer)
inline bool ptr_on_device(const sicp_ctx *c, const void *p)
{
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeDevice && at.device == c->device) return true;
    (void)hipGetLastError();
    return false;
}

// operators whose answer needs every point on this rank refuse an exchange (`who` is not supported ... (`why`)); check_whole_cloud
// also refuses a shard in `slot` and 2^31 points or more (check_below_2_31)
int check_no_exchange(const sicp_ctx *c, const char *who, const char *why);
int check_below_2_31(const sicp_ctx *c, int slot, const char *who);
int check_whole_cloud(const sicp_ctx *c, int slot, const char *who, const char *why);
// which of the three candidate forms a whole-cloud operator call takes: a row list, a device mask, or the whole slot
struct Candidates {
    const int64_t *d_rows = nullptr;   // device: the candidates' rows (null: rows 0, 1, ... of the slot)
    const uint8_t *d_mask = nullptr;   // the masked form's mask, known to be memory of the ctx's device
    long count = 0;                    // candidates
    long positions = 0;                // entries of every output
    bool by_position = false;          // results go to the candidate's ROW (masked form), not to its place in the list
};
constexpr int CAND_WORDS = 8;          // c->cand_small, the counter words: [CAND_COUNT] belongs to take_candidates, the others to the operator
constexpr int CAND_COUNT = 5;          // the set bytes of a mask
// c->h_small, H_SMALL_WORDS pinned doubles.  The run's words lie below H_LOOP_END (sicp_icp.cpp: 8..37 normal equations, 128..159
// their polled copy, 160..175 statistics; sicp_clouds.cpp / sicp_device.hip: 40..46 cloud statistics, 54..55 grid build;
// sicp_search.cpp: 62 the filtered scan's overflow word); the stand-alone operators' follow
constexpr int H_SMALL_WORDS = 256, H_LOOP_END = 176;
constexpr int H_EVAL = 192, H_EVAL_WORDS = 12;   // sicp_evaluate's record
constexpr int H_CAND = 208;                      // the mirror of the counter words (counters_host)
static_assert(H_LOOP_END <= H_EVAL && H_EVAL + H_EVAL_WORDS <= H_CAND && H_CAND + CAND_WORDS <= H_SMALL_WORDS, "h_small's regions are apart");
// what a masked call does with its mask before anything else: enqueue the kernel that adds the number of set bytes to *d_count
// (zero before) and say in *d_rows where it collected their rows (null: it only counted)
typedef int (*MaskPass)(sicp_ctx *c, const uint8_t *mask, long n, unsigned long long *d_count, const int64_t **d_rows);
int take_candidates(sicp_ctx *c, int slot, const int64_t *rows, int64_t m, const uint8_t *mask, MaskPass by_mask, Candidates *K);

// ---- an operator call's frame ("An operator call's frame") ------------------------------------------------------------
// body(), and on failure the stream drained: whatever the call enqueued is over before its caller sees the error
template <class Body>
int op_run(sicp_ctx *c, Body &&body)
{
    const int rc = body();
    if (rc != SICP_OK) (void)hipStreamSynchronize(c->stream);
    return rc;
}
// the counter words: zeroed on the stream; copied to their pinned mirror on the stream; the mirror, good after sync(c)
inline int counters_clear(sicp_ctx *c)
{
    CHK(c->cand_small.reserve(CAND_WORDS));
    HIPCHK(hipMemsetAsync(c->cand_small.p, 0, CAND_WORDS * sizeof(unsigned long long), c->stream));
    return SICP_OK;
}
inline unsigned long long *counters_host(const sicp_ctx *c) { return (unsigned long long *)(c->h_small + H_CAND); }
inline int counters_fetch(sicp_ctx *c)
{
    HIPCHK(hipMemcpyAsync(counters_host(c), c->cand_small.p, CAND_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    return SICP_OK;
}
// `count` elements at p as the kernels read them: p itself if it is memory of the ctx's device, else a copy in `buf`
template <class T>
int stage_in(sicp_ctx *c, const T *p, size_t count, DevBuf<T> &buf, const T **dev)
{
    if (ptr_on_device(c, p)) { *dev = p; return SICP_OK; }
    CHK(buf.reserve(count));
    HIPCHK(hipMemcpyAsync(buf.p, p, count * sizeof(T), hipMemcpyDefault, c->stream));
    *dev = buf.p;
    return SICP_OK;
}
// where the kernels write `count` elements meant for p (null: nowhere): p itself or `buf`; stage_leave copies the staged ones out
template <class T>
int stage_out(sicp_ctx *c, T *p, size_t count, DevBuf<T> &buf, T **dev)
{
    if (!p || ptr_on_device(c, p)) { *dev = p; return SICP_OK; }
    CHK(buf.reserve(count));
    *dev = buf.p;
    return SICP_OK;
}
template <class T>
int stage_leave(sicp_ctx *c, T *p, size_t count, const T *dev)
{
    if (p && dev != p) HIPCHK(hipMemcpyAsync(p, dev, count * sizeof(T), hipMemcpyDefault, c->stream));
    return SICP_OK;
}

// ---- a pose operator's frame ("A pose operator's frame"): what the entries over matched rows src[c] <-> dst[c] share ----
constexpr int POSE_BLOCK = 256;                    // threads of the kernels with one thread per pose
constexpr int POSE_BEST_BLOCKS = 1024;             // grid limit of the best kernel: its workgroups stride from there on
constexpr int POSE_MAX_POSES_Y = 32768;            // grid limit of the poses' dimension: the workgroups stride from there on
enum { POSE_VOID = 0, POSE_BEST1 = 2, POSE_BEST = 3 };   // the shared counter words (BEST1 = max of inliers + 1); word 1 is the operator's
static_assert(POSE_BEST < CAND_WORDS && POSE_BEST != CAND_COUNT && POSE_BEST1 != CAND_COUNT, "the record's counters fit the ctx's counter words");
// the checks, in the order the entries make them
inline int check_rows_ctx(sicp_ctx *c, const char *who)
{
    if (!c) return fail(SICP_ERR_INVALID, "null ctx");
    return check_no_exchange(c, who, "the rows of one rank are not the job's");
}
inline int check_matched(const double *src, const double *dst)
{
    if (!src) return fail(SICP_ERR_INVALID, "src is null");
    if (!dst) return fail(SICP_ERR_INVALID, "dst is null");
    return SICP_OK;
}
inline int check_matched_count(int64_t m)
{
    if (m < 3) return fail(SICP_ERR_INVALID, "m must be >= 3 (%lld given)", (long long)m);
    if (m >= (1LL << 31)) return fail(SICP_ERR_INVALID, "m must be < 2^31 (%lld given)", (long long)m);
    return SICP_OK;
}
inline int check_poses_rounds(const double *poses_in, int64_t b, int rounds, int max_rounds)
{
    if (b < 1) return fail(SICP_ERR_INVALID, "b must be >= 1 (%lld given)", (long long)b);
    if (b >= (1LL << 31)) return fail(SICP_ERR_INVALID, "b must be < 2^31 (%lld given)", (long long)b);
    if (!poses_in && b != 1) return fail(SICP_ERR_INVALID, "poses_in is null: b must be 1 then (%lld given)", (long long)b);
    if (rounds < 1 || rounds > max_rounds) return fail(SICP_ERR_INVALID, "rounds must be >= 1 and <= %d (%d given)", max_rounds, rounds);
    return SICP_OK;
}
inline int check_max_distance(double max_distance, bool or_inf)
{
    if (or_inf) {
        if (std::isnan(max_distance) || !(max_distance > 0.0)) return fail(SICP_ERR_INVALID, "max_distance must be > 0 (finite or +inf)");
    } else if (!std::isfinite(max_distance) || !(max_distance > 0.0)) {
        return fail(SICP_ERR_INVALID, "max_distance must be finite and > 0");
    }
    return SICP_OK;
}
// the call's arrays as the kernels take them, and the counter words cleared: src and dst (m rows), poses_in (null, or n poses), the
// n poses (nullable) and n counts that leave
struct PoseRows {
    const double *src, *dst, *poses_in = nullptr;
    double *poses;
    int32_t *inl;
};
inline int pose_rows_enter(sicp_ctx *c, const double *src, const double *dst, int64_t m, const double *poses_in, int64_t n, double *poses_out,
                           int32_t *inliers_out, PoseRows *R)
{
    CHK(stage_in(c, src, (size_t)3 * m, c->gl_src, &R->src));
    CHK(stage_in(c, dst, (size_t)3 * m, c->gl_dst, &R->dst));
    if (poses_in) CHK(stage_in(c, poses_in, (size_t)12 * n, c->pf_in, &R->poses_in));
    CHK(stage_out(c, poses_out, (size_t)12 * n, c->gl_pose, &R->poses));
    CHK(stage_out(c, inliers_out, (size_t)n, c->gl_idx, &R->inl));
    CHK(counters_clear(c));
    HIPCHK(hipMemsetAsync(c->cand_small.p + POSE_BEST, 0xff, sizeof(unsigned long long), c->stream));
    return SICP_OK;
}
// ... behind the best kernel: the counters fetched, the staged outputs copied out, the stream drained; the record's shared fields
// (the operator's own word is counters_host(c)[1])
template <class Stats>
int pose_rows_leave(sicp_ctx *c, double *poses_out, int32_t *inliers_out, int64_t n, const PoseRows &R, Stats *out)
{
    CHK(counters_fetch(c));
    CHK(stage_leave(c, poses_out, (size_t)12 * n, R.poses));
    CHK(stage_leave(c, inliers_out, (size_t)n, R.inl));
    CHK(sync(c));
    const unsigned long long *hs = counters_host(c);
    out->n_void = (int64_t)hs[POSE_VOID];
    out->best = hs[POSE_BEST1] ? (int64_t)hs[POSE_BEST] : -1;
    out->best_inliers = (int64_t)hs[POSE_BEST1] - 1;
    return SICP_OK;
}
// the record's best index among the n counts at inl, by the unit's k_pose_best (sicp_pose_dev.h), enqueued behind the kernels that
// wrote them and the counter words: one grid rule for every operator
typedef void (*PoseBestKernel)(const int32_t *, long, unsigned long long *);
inline int pose_best_enqueue(sicp_ctx *c, PoseBestKernel best, const int32_t *inl, long n)
{
    void *args[] = {&inl, &n, &c->cand_small.p};
    HIPCHK(hipLaunchKernel((const void *)best, dim3(std::min(cdiv(n, (long)POSE_BLOCK), (unsigned)POSE_BEST_BLOCKS)), dim3(POSE_BLOCK), args, 0,
                           c->stream));
    return SICP_OK;
}
// the geometry of the sweeps over m rows and b poses: the tree's P, the spans of `span` rows and the level of `fold` above them, the
// grids of a first stage, of a second stage and of the kernels with one thread per pose
struct PoseGrids {
    long P, nb, nb2;
    dim3 sweep, fold, poses;
};
inline PoseGrids pose_grids(long m, long b, long span, long fold)
{
    PoseGrids G;
    G.P = 1;
    while (G.P < m) G.P *= 2;
    G.nb = cdiv(m, span);
    G.nb2 = cdiv(G.nb, fold);
    G.sweep = dim3((unsigned)G.nb, (unsigned)std::min<long>(b, POSE_MAX_POSES_Y));
    G.fold = dim3((unsigned)std::min<long>(b, POSE_MAX_POSES_Y));
    G.poses = dim3(cdiv(b, (long)POSE_BLOCK));
    return G;
}

// a chunked k-NN over rows of a slot (sicp_search.cpp): rows per search -- the ctx's switch, else as many as keep a chunk's
// (chunk, k) distances and indices at 256 MiB; c->kq / k_d2 / k_idx for chunks of up to `most` rows; rows d_rows[lo, lo + cnt)
// (null: rows lo, lo + 1, ...) as query columns in c->kq (stride round_up(cnt, QPAD)); ... searched: (cnt, k) in c->k_d2 / c->k_idx
long knn_chunk(long forced, int k);
int knn_chunk_reserve(sicp_ctx *c, long most, int k);
void rows_gather(sicp_ctx *c, int slot, const int64_t *d_rows, long lo, long cnt);
int rows_knn(sicp_ctx *c, int slot, const int64_t *d_rows, long lo, long cnt, int k);
// the rows sel_idx[0, Q) of a cloud (host or device memory, staged in `sel`; null: rows 0 .. Q - 1) as query columns in c->kq;
// *qpad_out: their stride
int selected_queries(sicp_ctx *c, const Cloud &cl, const int64_t *sel_idx, long Q, DevBuf<int64_t> &sel, long *qpad_out);
double key_to_double(unsigned long long k);
int subsample_build(sicp_ctx *c, int slot);
int grid_coarse_level(sicp_ctx *c, int slot, GridLevel *lv, const GridLevel **out);
int grid_companions(sicp_ctx *c, const Cloud &cl, Grid &gr, long n, bool want_recf, bool want_box);
int points_order_build(sicp_ctx *c, const double *qx, const double *qy, const double *qz, long cnt, double h, long max_cells,
                       DevBuf<uint32_t> &order);
int query_order_build(sicp_ctx *c, long lo, long cnt, double h);
bool rigid_inverse(const Xf &H, Xf *inv);
double smax3(const Xf &H);
int knn1_device(sicp_ctx *c, int slot, const double *qsoa, long Q, long qpad, const Xf *H, double max_dist,
                const double *prev_p2, double *d2_out, int64_t *idx_out, double *p2_out);
bool knnk_uses_grid(const sicp_ctx *c, const Cloud &cl, long Q);
int normal_eq_host(sicp_ctx *c, const double x[6], bool write_resid, bool allow_shard, double out[30]);
double objective(const double ne[30], double w, const double x[6], const double obs[6], const double ow[6]);
int grid_build_arrays(sicp_ctx *c, const Cloud &cl, const double *X, const double *Y, const double *Z, long n, Grid &gr, double target = 0.0,
                      double h_forced = 0.0);
int grid_build(sicp_ctx *c, int slot, long icp_queries = -1);
int knnk_device(sicp_ctx *c, int slot, const double *qsoa, long Q, long qpad, int k, double *d2_out, int64_t *idx_out,
                float *normals_out = nullptr, float *planarity_out = nullptr, bool *fused = nullptr);
int cloud_stats(sicp_ctx *c, int slot);
int cloud_stats_take(sicp_ctx *c, int slot, const unsigned long long hk[7]);
int upload_begin(sicp_ctx *c, int slot, int64_t n, int64_t index_base);
int upload_join(sicp_ctx *c, int slot);
int loop_state_init(sicp_ctx *c, const sicp_iter_params *P0);
int chain_prepare(sicp_ctx *c, const sicp_iter_params *P0, bool *grid, double *last_move);
TailArgs tail_args(const sicp_ctx *c, const sicp_iter_params *P0, double min_change);
int take_record(sicp_ctx *c, const sicp_iter_params *P0, const double *o, sicp_iter_result *results, int64_t *done_out,
                double xcur[6], double *last_move, bool *over);
bool device_tail(const sicp_ctx *c);
int check_iter_args(sicp_ctx *c, const sicp_iter_params *P);
int check_corr(sicp_ctx *c);
int corr_alive_stats(sicp_ctx *c, const double *also4, double **h_st_out);
// rejection by the angle between normals (sicp_nangle.hip): is the ctx's setting on; a run's / an iteration's preparation (buffers,
// cache, counters); one iteration's launches on c->flag -- H from the chained run's loop state `st`, or by value
bool normal_angle_on(const sicp_ctx *c);
int normal_angle_prepare(sicp_ctx *c);
int normal_angle_enqueue(sicp_ctx *c, const IcpDev *st, const Xf *H);

}  // namespace sicph

#endif
