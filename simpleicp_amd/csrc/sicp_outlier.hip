// sicp_outlier.hip -- outlier removal (include/simpleicp_hip_outlier.h; contract (O)).
//
// Statistical filter: the candidates go through the slot's k-NN search (knnk_device: the one-sweep kernel on the grid, in cell
// order) a chunk at a time, k_ol_mean turns a chunk's ranked (chunk, k) squared distances into d_i at the candidate's POSITION;
// two trees over all positions (k_ol_partials / k_ol_fold: contract (E)'s adjacent-pair tree of one term, sicp_pairtree.h) give mean
// and std, k_ol_verdict writes the bytes and counts them.
// Radius filter: k_ball_count walks the grid rows of a candidate's ball (ball_walk: sicp_ball_dev.h), counts d2 < r^2 and leaves at
// min_points + 1.  Integer atomics count; no floating-point atomic takes part.
#include "sicp_host.h"
#include "sicp_ball_dev.h"
#include "sicp_pairtree.h"
#include "../../include/simpleicp_hip_outlier.h"

namespace sicp {
namespace {

constexpr int OL_BLOCK = 256;
constexpr int OL_MAX_BLOCKS = 4096;

// st: [0] mean [1] std [2] threshold.  SQ false: term = d (non-candidates hold +0.0 there); true: (d - mean)^2 of the candidates
template <bool SQ>
__global__ __launch_bounds__(PT_BLOCK) void k_ol_partials(const double *__restrict__ d, const uint8_t *__restrict__ mask, long n, long P,
                                                          const double *__restrict__ st, double *__restrict__ part)
{
    __shared__ double node[PT_TILES * PT_WAVES][1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long base = (long)blockIdx.x * PT_SPAN;
    const double mean = SQ ? st[0] : 0.0;
#pragma unroll
    for (int t = 0; t < PT_TILES; ++t) {
        const long e = base + (long)t * PT_BLOCK + threadIdx.x;
        double v[1] = {0.0};
        if (e < n) {
            const double di = d[e];
            if (SQ) {
                const double c = di - mean;
                v[0] = (!mask || mask[e] != 0) ? c * c : 0.0;
            } else {
                v[0] = di;
            }
        }
        pt_wave(v, e, P);
        if (lane == 0) node[t * PT_WAVES + wave][0] = v[0];
    }
    const double s = pt_nodes<PT_TILES * PT_WAVES>(node, base, P);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// One workgroup: the tree over the nb partials (pt_fold, between the buffers a and b); then the statistics.
// SQ false: st[0] = sum / m; true: st[1] = sqrt(sum / (m - 1)) (m == 1: 0), st[2] = st[0] + ratio * st[1].
template <bool SQ>
__global__ __launch_bounds__(PT_FOLD) void k_ol_fold(double *a, double *b, long nb, double m, double ratio, double *__restrict__ st)
{
    __shared__ double node[PT_FOLD_WAVES][1];
    long sa = 0;                                                   // (one term: one row)
    pt_fold(a, sa, b, 0, nb, node);
    if (threadIdx.x == 0) {
        const double sum = a[0];
        if (!SQ) {
            st[0] = sum / m;
        } else {
            const double sd = m > 1.0 ? sqrt(sum / (m - 1.0)) : 0.0;
            const double w = ratio * sd;
            st[1] = sd;
            st[2] = st[0] + w;
        }
    }
}

// d_i of the Q candidates of a chunk from their ranked squared distances: d[pos] = (sqrt(d2_0) + ... + sqrt(d2_(k-1))) / k
__global__ __launch_bounds__(OL_BLOCK) void k_ol_mean(const double *__restrict__ d2, long Q, int k, const int64_t *__restrict__ pos,
                                                      double *__restrict__ d)
{
    const long q = (long)blockIdx.x * OL_BLOCK + threadIdx.x;
    if (q >= Q) return;
    const double *row = d2 + q * k;
    double s = sqrt(row[0]);
    for (int j = 1; j < k; ++j) s = s + sqrt(row[j]);
    d[pos ? pos[q] : q] = s / (double)k;
}

// keep[e] = candidate and d[e] <= threshold; cnt[0] += the kept
__global__ __launch_bounds__(OL_BLOCK) void k_ol_verdict(const double *__restrict__ d, const uint8_t *__restrict__ mask, long n,
                                                         const double *__restrict__ st, uint8_t *__restrict__ keep,
                                                         unsigned long long *__restrict__ cnt)
{
    const double thr = st[2];
    const long stride = (long)gridDim.x * OL_BLOCK;
    unsigned mine = 0;                                             // (n < 2^31)
    for (long e = (long)blockIdx.x * OL_BLOCK + threadIdx.x; e < n; e += stride) {
        const bool k = (!mask || mask[e] != 0) && d[e] <= thr;
        keep[e] = k ? 1 : 0;
        mine += k ? 1u : 0u;
    }
    mine = wsum_u32(mine);                                         // block_sum_u32's wave step: one atomic per wave
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(cnt, (unsigned long long)mine);
}

// rows[0 .. *cnt) = the points whose mask byte is set (in no particular order: every result lands at the point's own position)
__global__ __launch_bounds__(OL_BLOCK) void k_ol_compact(const uint8_t *__restrict__ mask, long n, int64_t *__restrict__ rows,
                                                         unsigned long long *__restrict__ cnt)
{
    const long stride = (long)gridDim.x * OL_BLOCK;
    const long rounds = (n + stride - 1) / stride;             // (every lane of a wave takes every round: the ballot is wave-wide)
    for (long r = 0; r < rounds; ++r) {
        const long e = r * stride + (long)blockIdx.x * OL_BLOCK + threadIdx.x;
        const bool set = e < n && mask[e] != 0;
        const unsigned long long at = wave_append(cnt, set);
        if (set) rows[at] = e;
    }
}

// ---- the radius filter -----------------------------------------------------------------------------------------------------------
// BALL_GS lanes per candidate (ball_group_point, ball_walk: sicp_ball_dev.h).  A candidate leaves as soon as its count reaches cap.
// pos: where candidate q's results go (null: q); order: the candidates in cell order.
__global__ __launch_bounds__(BALL_BLOCK) void k_ball_count(const double *__restrict__ qx, const double *__restrict__ qy,
                                                           const double *__restrict__ qz, const uint32_t *__restrict__ order,
                                                           const int64_t *__restrict__ pos, const uint32_t *__restrict__ cell_start,
                                                           const double4 *__restrict__ rec, long Q, GridGeom G, double r, double r2,
                                                           unsigned cap, uint8_t *__restrict__ keep, uint32_t *__restrict__ cnt_out,
                                                           unsigned long long *__restrict__ kept_total, unsigned long long *__restrict__ work)
{
    const int lane = threadIdx.x & 63, sub = lane & (BALL_GS - 1), gbase = lane & ~(BALL_GS - 1);
    const long q = ball_group_point(order, Q);
    const bool active = q >= 0;                                // (a group without a candidate still takes part in the wave's ballot below)
    bool kept = false;
    BallTally tally;
    if (active) {
        unsigned count = 0;
        ball_walk(cell_start, rec, G, qx[q], qy[q], qz[q], r, r2, sub, gbase, [&](bool h0, uint32_t, bool h1, uint32_t) {
            const unsigned m0 = (unsigned)(__ballot(h0) >> gbase) & ((1u << BALL_GS) - 1u);
            const unsigned m1 = (unsigned)(__ballot(h1) >> gbase) & ((1u << BALL_GS) - 1u);
            count += (unsigned)__popc(m0) + (unsigned)__popc(m1);
            return count < cap ? cap - count : 0u;
        }, work != nullptr, tally);
        if (count > cap) count = cap;
        kept = count >= cap;                                   // count_i > min_points
        if (sub == 0) {
            const long p = pos ? (long)pos[q] : q;
            keep[p] = kept ? 1 : 0;
            cnt_out[p] = count;
        }
    }
    const unsigned long long kb = __ballot(active && sub == 0 && kept);
    if (lane == 0 && kb && kept_total) atomicAdd(kept_total, (unsigned long long)__popcll((long long)kb));   // (null: the caller counts for itself)
    if (work) {
        const unsigned long long n_cand = wsum_u64(tally.cand), n_rows = wsum_u64(tally.rows);
        if (lane == 0) { atomicAdd(work, n_cand); atomicAdd(work + 1, n_rows); }
    }
}

}  // namespace
}  // namespace sicp

namespace {

enum { OL_MEAN = 0, OL_STD = 1, OL_THR = 2, OL_KEPT = 4 };     // counter words (CAND_COUNT is the intake's)
static_assert(OL_KEPT != CAND_COUNT && OL_THR < CAND_COUNT && OL_KEPT < CAND_WORDS, "the filters' words and the intake's are apart");

// what both filters check alike
int ol_common(sicp_ctx *c, int slot, const int64_t *rows, int64_t m, const uint8_t *mask, const void *keep_out, const char *who)
{
    CHK(check_slot(c, slot, true));
    if (!keep_out) return fail(SICP_ERR_INVALID, "keep_out is null");
    if (rows && mask) return fail(SICP_ERR_INVALID, "rows and mask are mutually exclusive");
    CHK(check_whole_cloud(c, slot, who, "a point's neighbours may live on another rank"));
    return check_candidate_rows(rows, m, c->cloud[slot].n);
}

// the masked form collects the rows of the set bytes: every result lands at the point's own position
int ol_compact_mask(sicp_ctx *c, const uint8_t *mask, long n, unsigned long long *d_count, const int64_t **d_rows)
{
    CHK(c->cand_rows.reserve((size_t)n));
    const unsigned g = std::min(cdiv(n, OL_BLOCK), (unsigned)OL_MAX_BLOCKS);
    hipLaunchKernelGGL(k_ol_compact, dim3(g), dim3(OL_BLOCK), 0, c->stream, mask, n, c->cand_rows.p, d_count);
    *d_rows = c->cand_rows.p;
    return SICP_OK;
}

// the outputs always leave through staging buffers, host or device memory alike (no stage_out): keep_out may alias the mask
int ol_deliver(sicp_ctx *c, void *dst, const void *src, size_t bytes)
{
    if (dst && bytes) HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, c->stream));
    return SICP_OK;
}

// extent of the ball's box of cells on a grid of cell size h, per axis and in all
long ol_box_cells(const GridGeom &G, double radius, int64_t ext[3])
{
    long cells = 1;
    for (int a = 0; a < 3; ++a) {
        const double w = std::floor(2.0 * radius * G.inv_h) + 3.0;
        ext[a] = w < (double)G.dim[a] ? (int64_t)w : (int64_t)G.dim[a];
        cells = cells > (1L << 40) ? cells : cells * (long)ext[a];
    }
    return cells;
}

// the grid level the radius filter walks: the slot's own grid, always (a coarse twin would admit 512 x the volume per cell counted:
// the limit on the box is what bounds a candidate's work, so it is taken on the grid the points were binned for)
int ol_level(sicp_ctx *c, int slot, double radius, GridLevel *lv, int64_t ext[3], long *cells)
{
    CHK(grid_build(c, slot));
    Cloud &cl = c->cloud[slot];
    lv->g = cl.grid.g; lv->cell_start = cl.grid.cell_start.p; lv->rec = cl.grid.rec.p;
    *cells = ol_box_cells(lv->g, radius, ext);
    return SICP_OK;
}

}  // namespace

namespace sicph {

// The radius filter's walk, for the units that count the same balls (sicp_cluster.hip; declared in sicp_host.h).
// ball_level: the grid level a ball of `radius` is walked on, refused where its box of cells exceeds SICP_OUTLIER_MAX_BOX_CELLS.
int ball_level(sicp_ctx *c, int slot, double radius, GridLevel *lv)
{
    int64_t ext[3]; long cells = 0;
    CHK(ol_level(c, slot, radius, lv, ext, &cells));
    if (cells > SICP_OUTLIER_MAX_BOX_CELLS)
        return fail(SICP_ERR_INVALID, "radius %g spans a box of %lld x %lld x %lld = %lld grid cells (cell size %g): at most %d -- choose a "
                    "smaller radius", radius, (long long)ext[0], (long long)ext[1], (long long)ext[2], (long long)cells, lv->g.h,
                    SICP_OUTLIER_MAX_BOX_CELLS);
    return SICP_OK;
}

int BallChunks::reserve()
{
    return c->kq.reserve((size_t)3 * round_up(std::min(chunk, std::max<long>(n, 1)), QPAD));
}

int BallChunks::enter(long lo, long cnt)
{
    if (kept) return SICP_OK;
    qpad = round_up(cnt, QPAD);
    rows_gather(c, slot, d_rows, lo, cnt);
    order = nullptr;
    if (c->order_min_q > 0 && cnt >= c->order_min_q) {
        CHK(points_order_build(c, c->kq.p, c->kq.p + qpad, c->kq.p + 2 * qpad, cnt, 2.0 * lv.g.h, 1L << 22, c->k_order));
        order = c->k_order.p;
    }
    kept = n <= chunk;
    return SICP_OK;
}

unsigned BallChunks::grid(long cnt) const
{
    const unsigned g = cdiv(cnt, BALL_BLOCK / BALL_GS);
    return order ? (g + 7u) & ~7u : g;                             // (ball_group_point: an eighth of the ordered points per XCD)
}

// ball_count_enqueue: k_ball_count over the cnt candidates of the chunk W stands in (pos: null, or where each candidate's results
// go): keep = count >= cap, cnt_out = min(count, cap), *kept_total += the kept (one atomic per wave that kept any, all on that one
// word; null: not counted).
int ball_count_enqueue(const BallChunks &W, const int64_t *pos, long cnt, double radius, unsigned cap, uint8_t *keep, uint32_t *cnt_out,
                       unsigned long long *kept_total)
{
    sicp_ctx *c = W.c;
    hipLaunchKernelGGL(k_ball_count, dim3(W.grid(cnt)), dim3(BALL_BLOCK), 0, c->stream, W.qx(), W.qy(), W.qz(), W.order, pos,
                       W.lv.cell_start, (const double4 *)W.lv.rec, cnt, W.lv.g, radius, radius * radius, cap, keep, cnt_out, kept_total,
                       c->count_work ? c->match_work.p : nullptr);
    HIPCHK(hipGetLastError());
    return SICP_OK;
}

}  // namespace sicph

SICP_EXPORT int sicp_outlier_version(void) { return SICP_OUTLIER_VERSION; }

SICP_EXPORT int sicp_outlier_statistical(sicp_ctx *c, int slot, const int64_t *rows, int64_t m, const uint8_t *mask, int k,
                                         double std_ratio, uint8_t *keep_out, double *mean_dist_out, sicp_outlier_stats *out)
{
    CHK(ol_common(c, slot, rows, m, mask, keep_out, "the statistical filter"));
    if (!out) return fail(SICP_ERR_INVALID, "out is null");
    Cloud &cl = c->cloud[slot];
    if (k < 2) return fail(SICP_ERR_INVALID, "k must be >= 2 (%d given)", k);
    if (k > SICP_OUTLIER_MAX_K) return fail(SICP_ERR_INVALID, "k must be <= %d (%d given)", SICP_OUTLIER_MAX_K, k);
    if (k > cl.n) return fail(SICP_ERR_INVALID, "k (%d) exceeds the number of points (%lld)", k, (long long)cl.n);
    if (!std::isfinite(std_ratio)) return fail(SICP_ERR_INVALID, "std_ratio must be finite");
    HIPCHK(hipSetDevice(c->device));
    return op_run(c, [&]() -> int {
        Candidates K;
        CHK(take_candidates(c, slot, rows, m, mask, ol_compact_mask, &K));
        const long N = K.positions;
        CHK(c->cand_keep.reserve((size_t)N));
        CHK(c->ol_d.reserve((size_t)N));
        std::memset(out, 0, sizeof *out);
        if (K.count == 0) {                                        // an all-zero mask
            HIPCHK(hipMemsetAsync(c->cand_keep.p, 0, (size_t)N, c->stream));
            HIPCHK(hipMemsetAsync(c->ol_d.p, 0, (size_t)N * sizeof(double), c->stream));
            CHK(ol_deliver(c, keep_out, c->cand_keep.p, (size_t)N));
            CHK(ol_deliver(c, mean_dist_out, c->ol_d.p, (size_t)N * sizeof(double)));
            return sync(c);
        }
        if (K.by_position) HIPCHK(hipMemsetAsync(c->ol_d.p, 0, (size_t)N * sizeof(double), c->stream));   // +0.0 where no candidate is
        const long chunk = knn_chunk(c->outlier_chunk, k);
        CHK(knn_chunk_reserve(c, std::min(chunk, K.count), k));
        for (long lo = 0; lo < K.count; lo += chunk) {
            const long cnt = std::min(chunk, K.count - lo);
            CHK(rows_knn(c, slot, K.d_rows, lo, cnt, k));
            hipLaunchKernelGGL(k_ol_mean, dim3(cdiv(cnt, OL_BLOCK)), dim3(OL_BLOCK), 0, c->stream, c->k_d2.p, cnt, k,
                               K.by_position ? K.d_rows + lo : nullptr, K.by_position ? c->ol_d.p : c->ol_d.p + lo);
            HIPCHK(hipGetLastError());
        }
        // the two trees over all positions, then the verdicts
        const long nb = cdiv(N, PT_SPAN), nb2 = cdiv(nb, PT_FOLD);
        long P = 1;
        while (P < N) P *= 2;
        CHK(c->ol_part.reserve((size_t)(nb + nb2)));
        double *st = (double *)c->cand_small.p;
        const double md = (double)K.count;
        hipLaunchKernelGGL(k_ol_partials<false>, dim3((unsigned)nb), dim3(PT_BLOCK), 0, c->stream, c->ol_d.p, K.d_mask, N, P, st, c->ol_part.p);
        hipLaunchKernelGGL(k_ol_fold<false>, dim3(1), dim3(PT_FOLD), 0, c->stream, c->ol_part.p, c->ol_part.p + nb, nb, md, std_ratio, st);
        hipLaunchKernelGGL(k_ol_partials<true>, dim3((unsigned)nb), dim3(PT_BLOCK), 0, c->stream, c->ol_d.p, K.d_mask, N, P, st, c->ol_part.p);
        hipLaunchKernelGGL(k_ol_fold<true>, dim3(1), dim3(PT_FOLD), 0, c->stream, c->ol_part.p, c->ol_part.p + nb, nb, md, std_ratio, st);
        const unsigned g = std::min(cdiv(N, OL_BLOCK), (unsigned)OL_MAX_BLOCKS);
        hipLaunchKernelGGL(k_ol_verdict, dim3(g), dim3(OL_BLOCK), 0, c->stream, c->ol_d.p, K.d_mask, N, st, c->cand_keep.p, c->cand_small.p + OL_KEPT);
        HIPCHK(hipGetLastError());
        CHK(counters_fetch(c));
        CHK(ol_deliver(c, keep_out, c->cand_keep.p, (size_t)N));
        CHK(ol_deliver(c, mean_dist_out, c->ol_d.p, (size_t)N * sizeof(double)));
        CHK(sync(c));
        const unsigned long long *h = counters_host(c);
        out->n_candidates = (int64_t)K.count;
        out->n_kept = (int64_t)h[OL_KEPT];
        std::memcpy(&out->mean, h + OL_MEAN, sizeof(double));
        std::memcpy(&out->std, h + OL_STD, sizeof(double));
        std::memcpy(&out->threshold, h + OL_THR, sizeof(double));
        return SICP_OK;
    });
}

SICP_EXPORT int sicp_outlier_radius_cells(sicp_ctx *c, int slot, double radius, int64_t out4[4])
{
    CHK(check_slot(c, slot, true));
    if (!out4) return fail(SICP_ERR_INVALID, "out4 is null");
    if (!std::isfinite(radius) || !(radius > 0.0)) return fail(SICP_ERR_INVALID, "radius must be finite and > 0");
    CHK(check_below_2_31(c, slot, "the radius filter"));
    HIPCHK(hipSetDevice(c->device));
    GridLevel lv; long cells = 0;
    CHK(ol_level(c, slot, radius, &lv, out4, &cells));
    out4[3] = (int64_t)cells;
    return SICP_OK;
}

SICP_EXPORT int sicp_outlier_radius(sicp_ctx *c, int slot, const int64_t *rows, int64_t m, const uint8_t *mask, double radius,
                                    int64_t min_points, uint8_t *keep_out, uint32_t *count_out, int64_t *kept_out)
{
    CHK(ol_common(c, slot, rows, m, mask, keep_out, "the radius filter"));
    if (!kept_out) return fail(SICP_ERR_INVALID, "kept_out is null");
    if (!std::isfinite(radius) || !(radius > 0.0)) return fail(SICP_ERR_INVALID, "radius must be finite and > 0");
    if (min_points < 0) return fail(SICP_ERR_INVALID, "min_points must be >= 0");
    HIPCHK(hipSetDevice(c->device));
    return op_run(c, [&]() -> int {
        GridLevel lv;
        CHK(ball_level(c, slot, radius, &lv));
        Candidates K;
        CHK(take_candidates(c, slot, rows, m, mask, ol_compact_mask, &K));
        const long N = K.positions;
        CHK(c->cand_keep.reserve((size_t)N));
        CHK(c->ol_cnt.reserve((size_t)N));
        if (K.by_position) {
            HIPCHK(hipMemsetAsync(c->cand_keep.p, 0, (size_t)N, c->stream));
            HIPCHK(hipMemsetAsync(c->ol_cnt.p, 0, (size_t)N * sizeof(uint32_t), c->stream));
        }
        const unsigned cap = (unsigned)std::min<int64_t>(min_points, (1LL << 31) - 1) + 1u;      // counts stay below 2^31
        BallChunks W{c, slot, lv, K.d_rows, K.count, c->outlier_chunk > 0 ? c->outlier_chunk : (1L << 22)};
        CHK(W.reserve());
        for (long lo = 0; lo < K.count; lo += W.chunk) {
            const long cnt = std::min(W.chunk, K.count - lo);
            CHK(W.enter(lo, cnt));
            CHK(ball_count_enqueue(W, K.by_position ? K.d_rows + lo : nullptr, cnt, radius, cap,
                                   K.by_position ? c->cand_keep.p : c->cand_keep.p + lo, K.by_position ? c->ol_cnt.p : c->ol_cnt.p + lo,
                                   c->cand_small.p + OL_KEPT));
        }
        CHK(counters_fetch(c));
        CHK(ol_deliver(c, keep_out, c->cand_keep.p, (size_t)N));
        CHK(ol_deliver(c, count_out, c->ol_cnt.p, (size_t)N * sizeof(uint32_t)));
        CHK(sync(c));
        *kept_out = (int64_t)counters_host(c)[OL_KEPT];
        return SICP_OK;
    });
}
