// sicp_ball_dev.h -- "who is within r of this point", for the kernels that answer it over the dense cell table with one arithmetic
// contract (device code only): k_ball_count (sicp_outlier.hip), k_ball_union and k_ball_border (sicp_cluster.hip).  A group of
// BALL_GS lanes takes one point (ball_group_point) and walks the rows of its ball's box of cells (ball_walk); what a kernel does
// with the neighbours is its visitor.  The host's side of the same rules is BallChunks (sicp_host.h, sicp_outlier.hip).
#ifndef SICP_BALL_DEV_H
#define SICP_BALL_DEV_H

#include "sicp_grid_dev.h"

namespace sicp {

constexpr int BALL_BLOCK = 256;                    // threads per workgroup of the three kernels
constexpr int BALL_GS = 16;                        // lanes per point (k_grid_nn16's share of a wave: a group is one DPP row and talks through ballots and ds_bpermute)

// Which point a group of BALL_GS lanes takes: slot s of the launch -- point s, or order[s] where the points come in cell order; one
// contiguous eighth of the ordered points per XCD then (the grid is a multiple of 8 blocks: BallChunks::grid).  -1: none.
__device__ __forceinline__ long ball_group_point(const uint32_t *__restrict__ order, long Q)
{
    long blk = blockIdx.x;
    if (order) {
        const long per_xcd = gridDim.x >> 3;
        blk = (long)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    }
    const long slot = blk * (BALL_BLOCK / BALL_GS) + (threadIdx.x / BALL_GS);
    if (slot >= Q) return -1;
    return order ? (long)order[slot] : slot;
}

// what an instrumented walk tallies (sicp_timing_enable(ctx, 2)): candidates evaluated, rows with records
struct BallTally { unsigned long long cand = 0, rows = 0; };

// The walk of the ball of radius r around (ax, ay, az) by the BALL_GS lanes of a group (sub: the lane in its group, gbase: the
// group's first lane in the wave).  The ball's box of cells is walked row by row ((cy, cz) rows are contiguous in the cell order):
// the lanes fetch the record ranges of BALL_GS rows at once, culled to the ball along x (row_lb2, row_x_clip, row_records), then take
// the records of one row after the other, two per lane and step.
// hit(h0, j0, h1, j1), called by all lanes of the group together: is the lane's record a neighbour (d2 < r2, contract (D)), and its
// original index.  Its result, the same in every lane of the group: how many more neighbours the group wants -- 0 ends the walk (a
// number, not a flag, and the tally's sums in locals: what other forms cost k_ball_count is in profiles/radius_walk/README.md).
// tally: an instrumented launch -- t is added to.  The form below tallies nothing.
template <class Hit>
__device__ __forceinline__ void ball_walk(const uint32_t *__restrict__ cell_start, const double4 *__restrict__ rec, const GridGeom &G,
                                          double ax, double ay, double az, double r, double r2, int sub, int gbase, Hit &&hit,
                                          bool tally, BallTally &t)
{
    const double c3[3] = {ax, ay, az};
    // d2 < r2 implies |difference| < r along every axis up to the rounding of the difference itself: the ball that is culled with
    // is wider by that, and by the rounding of c - rr
    const double rr = r + (1e-9 * r + 1e-15 * (fabs(ax) + fabs(ay) + fabs(az) + r));
    const double rr2 = rr * rr, etol = 1e-6 * G.h;
    int lo[3], hi[3];
    // ball_block's text (sicp_grid_dev.h) without `all`, written out: measured with the three search kernels that keep theirs (profiles/ballwalk)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double fl = floor((c3[a] - rr - G.mn[a]) * G.inv_h - 1e-6);
        const double fh = floor((c3[a] + rr - G.mn[a]) * G.inv_h + 1e-6);
        lo[a] = fl < 0.0 ? 0 : (fl > (double)(G.dim[a] - 1) ? G.dim[a] - 1 : (int)fl);
        hi[a] = fh < 0.0 ? 0 : (fh > (double)(G.dim[a] - 1) ? G.dim[a] - 1 : (int)fh);
    }
    const int ny = hi[1] - lo[1] + 1, nz = hi[2] - lo[2] + 1;
    const int nrows = ny * nz;                                 // (the host bounds the box: SICP_OUTLIER_MAX_BOX_CELLS)
    unsigned left = 1u;
    unsigned long long n_cand = 0, n_rows = 0;
    for (int rb = 0; rb < nrows && left != 0u; rb += BALL_GS) {
        uint32_t b = 0, len = 0;
        const int rw = rb + sub;
        if (rw < nrows) {
            const int oz = rw / ny, oy = rw - oz * ny;
            const int cy = lo[1] + oy, cz = lo[2] + oz;
            const long row = ((long)cz * G.dim[1] + cy) * G.dim[0];
            const double rem = rr2 - row_lb2(G, cy, cz, ay, az, etol);
            if (rem >= 0.0) {                                  // (row_x_clip's own test, here too: the compiler's allocation, two VGPRs)
                int xl = lo[0], xh = hi[0];
                row_x_clip(G, ax, rem, etol, xl, xh);
                row_records(cell_start, row, xl, xh, b, len);
            }
        }
        unsigned todo = (unsigned)(__ballot(len > 0) >> gbase) & ((1u << BALL_GS) - 1u);
        if (tally) n_rows += len > 0 ? 1 : 0;
        while (todo && left != 0u) {
            const int j = __ffs((int)todo) - 1;
            todo &= todo - 1u;
            const uint32_t bj = (uint32_t)__shfl((int)b, gbase + j), lj = (uint32_t)__shfl((int)len, gbase + j);
            for (uint32_t o = 0; o < lj && left != 0u; o += 2 * BALL_GS) {
                const uint32_t i0 = o + (uint32_t)sub, i1 = i0 + BALL_GS;
                const bool ok0 = i0 < lj, ok1 = i1 < lj;
                const double4 P0 = rec[ok0 ? bj + i0 : bj], P1 = rec[ok1 ? bj + i1 : bj];
                const double dx0 = P0.x - ax, dy0 = P0.y - ay, dz0 = P0.z - az;
                const double dx1 = P1.x - ax, dy1 = P1.y - ay, dz1 = P1.z - az;
                const bool h0 = ok0 && fma(dz0, dz0, fma(dy0, dy0, dx0 * dx0)) < r2;
                const bool h1 = ok1 && fma(dz1, dz1, fma(dy1, dy1, dx1 * dx1)) < r2;
                left = hit(h0, (uint32_t)__double_as_longlong(P0.w), h1, (uint32_t)__double_as_longlong(P1.w));
                if (tally) n_cand += (ok0 ? 1 : 0) + (ok1 ? 1 : 0);
            }
        }
    }
    t.cand += n_cand; t.rows += n_rows;
}

template <class Hit>
__device__ __forceinline__ void ball_walk(const uint32_t *__restrict__ cell_start, const double4 *__restrict__ rec, const GridGeom &G,
                                          double ax, double ay, double az, double r, double r2, int sub, int gbase, Hit &&hit)
{
    BallTally none;
    ball_walk(cell_start, rec, G, ax, ay, az, r, r2, sub, gbase, hit, false, none);
}

}  // namespace sicp

#endif
