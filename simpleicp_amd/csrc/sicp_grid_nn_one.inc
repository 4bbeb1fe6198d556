// sicp_grid_nn_one.inc -- the search of ONE query by one wave: the body of k_grid_nn's per-query lambda, included textually by
// k_grid_nn (sicp_grid.hip) and by the batched match k_grid_nn_batch, so that both compile the same tokens (a shared __device__
// function changed k_grid_nn's register allocation).  Names it uses: the kernel's parameters (st, qx, qy, qz, prev_p2, cell_start,
// rec, G, H, Hinv, rmax, max_d2, idx_base, d2_out, idx_out, p2_out, work, post, G2, rec2), the locals lane, tight, approx,
// cell_box, cell_start2, redo_list, and q, the query.  XFORM, CHAINED: the kernel's template parameters.  WAIT (a compile-time
// constant, with tkt and wait_seq): the launch was enqueued BEFORE the tail it follows has ended and waits for that tail's ticket
// (k_grid_nn_wait, sicp_grid.hip) -- everywhere else false, and the text below compiles to what it was.
    const double ax = qx[q], ay = qy[q], az = qz[q];      // (issued before the loop state is waited for)
    double px0 = 0, py0 = 0, pz0 = 0;
    if constexpr (!WAIT) { if (prev_p2) { px0 = prev_p2[3 * q]; py0 = prev_p2[3 * q + 1]; pz0 = prev_p2[3 * q + 2]; } }
    float pnx = 0.f, pny = 0.f, pnz = 0.f, ppl = 0.f;     // the query's normal and planarity (wave-uniform; in flight during the search)
    if (post.dist) { pnx = post.normals[3 * q]; pny = post.normals[3 * q + 1]; pnz = post.normals[3 * q + 2]; ppl = post.planarity[q]; }
    if constexpr (WAIT) {
        // The loads above are constant over a run (queries, normals, planarity: written before the run, and this launch's stream
        // waited for that) -- they are in flight while lane 0 of the workgroup's first wave polls the ticket; the other waves wait
        // at the barrier (waves past Q have ended: the barrier counts the live ones).  Bounded like grid_barrier's polling: a launch
        // that is never released stops the run (the tails behind it report status 4) instead of hanging the queue.
        if (threadIdx.x == 0) {
            long spins = 0;
            while (__hip_atomic_load(tkt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < wait_seq) {
                __builtin_amdgcn_s_sleep(4);
                if (++spins > (1L << 21)) {
                    // the stop flag first, complete before the error word: a poller that leaves on the error word finds stop set
                    __hip_atomic_store(reinterpret_cast<unsigned long long *>(const_cast<int *>(&st->done_iters)), 1ull << 32,
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __hip_atomic_store(tkt + PRE_ERR_WORD, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    break;
                }
                if ((spins & 1023) == 0 && __hip_atomic_load(tkt + PRE_ERR_WORD, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0ull) break;
            }
        }
        __syncthreads();
        // What an earlier launch wrote while this one was already running -- the loop state (H, its inverse, the stop flag: the
        // tail's agent-scope stores) and the previous match (its plain stores, written back when that kernel ended, before the tail
        // that published the ticket began) -- is read with agent-scope loads, performed at the coherence point: this XCD's L2 and
        // the scalar cache may hold lines from before the data existed (the wave's start-of-kernel invalidate came too early).
        // One load instruction each: lane l takes word l, the values reach the scalar registers by v_readlane.  Everything else the
        // search reads (the grid, the movable cloud's planarity) is as old as the run.
        static_assert(offsetof(IcpDev, H) == 96 && offsetof(IcpDev, Hinv) == 192 && offsetof(IcpDev, stop) == 316 && sizeof(Xf) == 96,
                      "the words lanes 0..27 load");
        const unsigned long long *sw = reinterpret_cast<const unsigned long long *>(st) + 12;
        const unsigned long long wv = __hip_atomic_load(sw + (lane < 28 ? lane : 27), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        unsigned long long pv = 0ull;
        if (prev_p2) pv = __hip_atomic_load(reinterpret_cast<const unsigned long long *>(prev_p2) + 3 * q + (lane < 3 ? lane : 2),
                                            __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned wlo = (unsigned)wv, whi = (unsigned)(wv >> 32);
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            H.m[i] = __hiloint2double(__builtin_amdgcn_readlane((int)whi, i), __builtin_amdgcn_readlane((int)wlo, i));
            Hinv.m[i] = __hiloint2double(__builtin_amdgcn_readlane((int)whi, 12 + i), __builtin_amdgcn_readlane((int)wlo, 12 + i));
        }
        if (__builtin_amdgcn_readlane((int)whi, 27) != 0) return;              // IcpDev::stop
        if (prev_p2) {
            const unsigned plo = (unsigned)pv, phi = (unsigned)(pv >> 32);
            px0 = __hiloint2double(__builtin_amdgcn_readlane((int)phi, 0), __builtin_amdgcn_readlane((int)plo, 0));
            py0 = __hiloint2double(__builtin_amdgcn_readlane((int)phi, 1), __builtin_amdgcn_readlane((int)plo, 1));
            pz0 = __hiloint2double(__builtin_amdgcn_readlane((int)phi, 2), __builtin_amdgcn_readlane((int)plo, 2));
        }
    } else if (CHAINED) {
        H = st->H; Hinv = st->Hinv;
        if (st->stop) return;
    }
    double cxq = ax, cyq = ay, czq = az;                  // query in the cloud's own frame
    if (XFORM) xf(Hinv, ax, ay, az, cxq, cyq, czq);
    // covers rounding of H^-1 q and |R^T R - I| ~ 1e-16: distances in the two frames agree to
    // ~1e-15 * scale; 1e-12 * scale leaves three orders of magnitude
    const double scale = rmax + (fabs(cxq) + fabs(cyq) + fabs(czq)) + 1.0;     // (1-norm: an upper bound of |q| is all the slack needs)
    const double slack = 1e-12 * scale;
    double r_lim = (max_d2 < __builtin_inf()) ? sqrt(max_d2) * (1.0 + 1e-12) + slack : __builtin_inf();
    bool lim_is_bound = false;                            // r_lim is the distance to a cloud point: that ball is never empty
    if (prev_p2) {
        double X = px0, Y = py0, Z = pz0;
        if (XFORM) { double u, v, w; xf(H, X, Y, Z, u, v, w); X = u; Y = v; Z = w; }
        const double dx = X - ax, dy = Y - ay, dz = Z - az;
        const double bnd = fma(dz, dz, fma(dy, dy, dx * dx));
        if (bnd < __builtin_inf()) {
            const double rb = sqrt(bnd) * (1.0 + 1e-12) + slack;
            if (rb < r_lim) { r_lim = rb; lim_is_bound = true; }
        }
    }
    // a bound that spans many cells (first iterations: the estimate still moves by metres) is not searched in one
    // go: start small and let the first hit shrink the ball
    double r = 0.75 * G.h;
    if (r > r_lim || (tight && r_lim < __builtin_inf())) r = r_lim;

    double best = __builtin_inf(), bx = 0, by = 0, bz = 0;
    uint32_t bidx = 0xffffffffu;
    unsigned long long n_cand = 0, n_rows = 0;
    bool last = false;
    for (int pass = 0; pass < 4096; ++pass) {                 // (ends by itself: the radius doubles until it hits, then one more pass)
        // A cloud whose density varies by orders of magnitude is binned for its dense core (cells of centimetres) -- and a query whose
        // answer lies metres away would walk ten thousand rows of that grid.  Such clouds carry a second, COARSE grid over the same
        // points (cells 8 x as wide): a pass whose ball spans more than a few fine cells runs on it.  Both grids hold every point, so
        // which one a pass reads changes what it costs, never what it finds.  (One query per wave: the choice is wave-uniform.)
        const bool cp = cell_start2 != nullptr && r > 4.0 * G.h;
        const GridGeom &Gp = cp ? G2 : G;
        const uint32_t *__restrict__ csp = cp ? cell_start2 : cell_start;
        const double4 *__restrict__ rcp = cp ? rec2 : rec;
        int lo[3], hi[3];
        const double c3[3] = {cxq, cyq, czq};
        // ball_block's text (sicp_grid_dev.h), written out: the compiler's allocation -- the call costs the EXT kernels two VGPRs,
        // k_grid_nn<true, *, true> its third wave (profiles/ballwalk/README.md)
        bool all = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double fl = floor((c3[a] - r - Gp.mn[a]) * Gp.inv_h - 1e-6);
            const double fh = floor((c3[a] + r - Gp.mn[a]) * Gp.inv_h + 1e-6);
            lo[a] = fl < 0.0 ? 0 : (fl > (double)(Gp.dim[a] - 1) ? Gp.dim[a] - 1 : (int)fl);
            hi[a] = fh < 0.0 ? 0 : (fh > (double)(Gp.dim[a] - 1) ? Gp.dim[a] - 1 : (int)fh);
            // whole axis covered <=> the ball reaches past both faces of the box
            all = all && (fl <= 0.0) && (fh >= (double)(Gp.dim[a] - 1));
        }
        best = __builtin_inf(); bidx = 0xffffffffu;
        const int ny = hi[1] - lo[1] + 1, nz = hi[2] - lo[2] + 1;
        const long nrows = (long)ny * nz;
        // candidates of up to four rows: ranges are wave-uniform, lane l takes record l (+ 64, ...) of each row
        auto scan_rows = [&](const uint32_t (&rbv)[4], const uint32_t (&rlv)[4]) {
            uint32_t longest = rlv[0] > rlv[1] ? rlv[0] : rlv[1];
            { const uint32_t t2 = rlv[2] > rlv[3] ? rlv[2] : rlv[3]; longest = longest > t2 ? longest : t2; }
            for (uint32_t o = 0; o < longest; o += 64) {              // (rows longer than a wave: dense cells, duplicates)
                double4 P[4];
                bool ok[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    ok[u] = o + (uint32_t)lane < rlv[u];
                    P[u] = rcp[ok[u] ? rbv[u] + o + (uint32_t)lane : 0u];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (!ok[u]) continue;
                    double X = P[u].x, Y = P[u].y, Z = P[u].z;
                    if (XFORM) { double a2, b2, c2; xf(H, X, Y, Z, a2, b2, c2); X = a2; Y = b2; Z = c2; }
                    const double dx = X - ax, dy = Y - ay, dz = Z - az;
                    const double d2 = fma(dz, dz, fma(dy, dy, dx * dx));
                    const uint32_t oi = (uint32_t)__double_as_longlong(P[u].w);
                    if (d2 < best || (d2 == best && oi < bidx)) { best = d2; bidx = oi; bx = P[u].x; by = P[u].y; bz = P[u].z; }
                }
                if (work) { for (int u = 0; u < 4; ++u) n_cand += ok[u] ? 1 : 0; }
            }
        };
        // The ball, not its bounding cube: a row (cy, cz) is needed only if its (y, z) rectangle comes within r of the query,
        // and then only the cells within sqrt(r^2 - lb^2) of it along x.  (`all`: the cube covers the whole grid and the pass
        // ends the search whatever it finds -- then every row is taken in full.)
        const double r2 = r * r, etol = 1e-6 * Gp.h;
        double cull2 = __builtin_inf();                           // rows farther than this cannot hold the answer (set by hits)
        const float inv_ny = 1.0f / (float)ny;
        const bool few_rows = nrows < (1L << 22);
        // row rr of the pass's block -> its cells [xl, xh] within the ball (the hit's, once there is one), its record range
        auto row_range = [&](long rr, uint32_t &b, uint32_t &len, double &lb2, long &row, int &cy, int &cz, int &xl, int &xh) {
            b = 0; len = 0;
            int oy, oz;
            row_split(rr, ny, inv_ny, few_rows, oy, oz);
            cy = lo[1] + oy; cz = lo[2] + oz;
            row = ((long)cz * Gp.dim[1] + cy) * Gp.dim[0];
            xl = lo[0]; xh = hi[0];
            lb2 = 0.0;
            if (!all) {
                lb2 = row_lb2(Gp, cy, cz, cyq, czq, etol);
                row_x_clip(Gp, cxq, fmin(r2, cull2) - lb2, etol, xl, xh);
            }
            if (lb2 <= cull2) row_records(csp, row, xl, xh, b, len);
        };
        for (long rb = 0; rb < nrows; rb += 64) {
            uint32_t b = 0, len = 0;
            double lb2 = __builtin_inf();
            long row = 0; int cy = 0, cz = 0, xl = 0, xh = -1;
            if (rb + lane < nrows) {
                row_range(rb + lane, b, len, lb2, row, cy, cz, xl, xh);
                // (a later batch of a far search: an earlier batch's hit already bounds the answer)
                if (cell_box && !cp && len > 0 && cull2 < __builtin_inf()) box_trim_row(cell_box, Gp, row, cy, cz, xl, xh, cxq, cyq, czq, cull2, etol, b, len);
            }
            unsigned long long todo = __ballot(len > 0);          // rows of this batch that hold points
            if (work && len > 0) n_rows += 1;                     // (per-lane tallies, summed once at the end)
            if (__popcll((long long)todo) > 4) {
                // many rows (a wide ball: cold start, far query): nearest row first, then drop the rows its hit rules out
                const unsigned long long key = len > 0 ? (unsigned long long)__double_as_longlong(lb2) : ~0ull, mk = gmin<64>(key);
                const int j = __ffsll((long long)__ballot(len > 0 && key == mk)) - 1;
                const uint32_t rbv[4] = {(uint32_t)__builtin_amdgcn_readlane((int)b, j), 0u, 0u, 0u};
                const uint32_t rlv[4] = {(uint32_t)__builtin_amdgcn_readlane((int)len, j), 0u, 0u, 0u};
                todo &= ~(1ull << j);
                scan_rows(rbv, rlv);
                const double wb = gmin<64>(best);
                if (wb < __builtin_inf()) {
                    const double rbnd = sqrt(wb) * (1.0 + 1e-12) + slack;
                    const double c2 = rbnd * rbnd;
                    if (c2 < cull2) {
                        cull2 = c2;
                        // the rows still to do: their cells within the HIT's ball, trimmed by the cells' tight boxes
                        if (cell_box && !cp && ((todo >> lane) & 1ull)) {
                            row_range(rb + lane, b, len, lb2, row, cy, cz, xl, xh);
                            if (len > 0) box_trim_row(cell_box, Gp, row, cy, cz, xl, xh, cxq, cyq, czq, cull2, etol, b, len);
                        }
                    }
                    todo &= __ballot(len > 0 && lb2 <= cull2);
                }
            }
            while (todo) {
                // up to four rows per step: ranges by register broadcast, one record per lane and row
                uint32_t rbv[4], rlv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    rbv[u] = 0; rlv[u] = 0;
                    if (todo) {
                        const int j = __ffsll((long long)todo) - 1;
                        todo &= todo - 1ull;
                        rbv[u] = (uint32_t)__builtin_amdgcn_readlane((int)b, j);
                        rlv[u] = (uint32_t)__builtin_amdgcn_readlane((int)len, j);
                    }
                }
                scan_rows(rbv, rlv);
            }
        }
        // wave-wide lexicographic (d2, original index) minimum: DPP butterfly, every lane ends up with it;
        // the lane that found it keeps the coordinates
        const double lbest = best; const uint32_t lidx = bidx;
        lexmin<64>(best, bidx);
        const bool found = bidx != 0xffffffffu;
        const bool winner = found && lbest == best && lidx == bidx;         // exactly one lane (indices are unique)
        // sqrt(best) + margin <= r, tested on the squares (no sqrt, no division).  The relative margin is HALF the one a
        // follow-up radius carries (r = sqrt(best) * (1 + 1e-12) + slack below), so the pass after a shrink terminates.
        const double r_eff = (r - slack) * (1.0 - 5e-13);
        const double r_eff2 = r_eff > 0.0 ? r_eff * r_eff * (1.0 - 1e-15) : -1.0;
        const bool done = (found && best <= r_eff2)           // nothing outside the ball can beat or tie it
                          || all || r >= r_lim                // searched everything that may qualify
                          || last                             // this ball was sized to hold the previous pass's hit: it holds the answer
                          || (approx && found);               // any cloud point will do
        if (done) {
            const bool ok = found && (best < max_d2);
            if (winner || (!found && lane == 0)) {
                d2_out[q] = ok ? best : __builtin_inf();
                const int64_t m = ok ? idx_base + (int64_t)bidx : (int64_t)-1;
                idx_out[q] = m;
                if (p2_out) {
                    p2_out[3 * q]     = ok ? bx : 0.0;
                    p2_out[3 * q + 1] = ok ? by : 0.0;
                    p2_out[3 * q + 2] = ok ? bz : 0.0;
                }
                if (post.dist) post_match(post, H, q, m, ok ? bx : 0.0, ok ? by : 0.0, ok ? bz : 0.0, ax, ay, az, pnx, pny, pnz, ppl);
                if (post.pack) {
                    double *r5 = post.pack + 5 * q;
                    r5[0] = ok ? best : __builtin_inf(); r5[1] = __longlong_as_double((long long)m);
                    r5[2] = ok ? bx : 0.0; r5[3] = ok ? by : 0.0; r5[4] = ok ? bz : 0.0;
                }
                if (post.pack_idx) post.pack_idx[q] = __longlong_as_double((long long)m);
            }
            break;
        }
        r = found ? sqrt(best) * (1.0 + 1e-12) + slack : 2.0 * r;
        last = found;
        if (r > r_lim) r = r_lim;
    }
    (void)lim_is_bound;
    if (work) {
        n_cand = wsum_u64(n_cand); n_rows = wsum_u64(n_rows);
        if (lane == 0) { atomicAdd(work, n_cand); atomicAdd(work + 1, n_rows); }
        if (q == 0 && lane == 0 && !redo_list) atomicAdd(work + 2, 1ull);
    }
