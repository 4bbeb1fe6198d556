// sicp_knn_sweep4.inc -- the body of the four-queries-per-wave k-NN sweep (sicp_grid.hip), shared by k_grid_knn_sweep4 (query count
// by value) and k_grid_knn_sweep4_list (query count read from device memory into Q before this body): the parameters are the
// including kernel's, see k_grid_knn_sweep4.
    extern __shared__ double ks_lds[];
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63, gl = lane & 15, gi = lane >> 4, gbase = lane & 48;
    const int kpad = (k + 7) & ~7;
    double *wbase = ks_lds + (size_t)(wid * 4 + gi) * kg_group_doubles(kpad);
    KnnKey *keys = (KnnKey *)wbase;               // (.pad: the candidate's record -- the k winners fetch their coordinates again, from L1 / L2;
    double *nbr = wbase + 2 * KG_CAP;             //  coordinates of all 64 survivors in LDS would cost two of five waves per SIMD)
    double *dk_slot = nbr + 3 * kpad;

    long blk = blockIdx.x;
    if (order) blk = (long)(blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);       // one contiguous eighth per XCD
    const long slot0 = ((blk * 4 + wid) * 4 + gi) * (long)batch;                            // this GROUP's first slot
    const int nb = slot0 >= Q ? 0 : (int)((Q - slot0 < (long)batch) ? (Q - slot0) : (long)batch);
    if (!__any(nb > 0)) return;
    uint32_t my_q = 0;
    if (gl < nb) my_q = order ? order[slot0 + gl] : (uint32_t)(slot0 + gl);
    const double inv_km1 = 1.0 / (double)(k - 1);
    const double etol = 1e-6 * G.h;
    double dk_est = (r_first * r_first) * (1.0 / (1.35 * 1.35));
    unsigned long long n_cand = 0, n_act = 0, n_defer = 0, n_surv = 0;

    for (int b = 0; b < batch; ++b) {
        const bool active = b < nb;
        const long q = active ? (long)(uint32_t)__shfl((int)my_q, gbase + b) : 0;
        const double ax = qx[q], ay = qy[q], az = qz[q];
        const double scale = rmax + (fabs(ax) + fabs(ay) + fabs(az)) + 1.0;
        const double slack = 1e-12 * scale;
        const double c3[3] = {ax, ay, az};
        double r = (double)(1.35f * sqrtf((float)dk_est)) + slack;
        if (!(r >= 0.25 * r_first)) r = 0.25 * r_first;
        int lo[3], hi[3];
        const bool all = ball_block(G, c3, r, lo, hi);
        const int ny = hi[1] - lo[1] + 1, nz = hi[2] - lo[2] + 1;
        const long nrows = (long)ny * nz;
        bool mine = active && !all && nrows <= 16;                 // this group does the query itself (so far)
        const double r_eff = (r - slack) * (1.0 - 1.5e-12);
        const double thr = r_eff > 0.0 ? r_eff * r_eff : -1.0;
        const double r2 = r * r;
        // ---- rows: lane gl takes row gl of the ball's (ny x nz) block ----
        uint32_t rbeg = 0, rlen = 0;
        if (mine && gl < (int)nrows) {
            int oy, oz;
            row_split((long)gl, ny, 1.0f / (float)ny, true, oy, oz);
            const int cy = lo[1] + oy, cz = lo[2] + oz;
            const long row = ((long)cz * G.dim[1] + cy) * G.dim[0];
            int xl = lo[0], xh = hi[0];
            row_x_clip(G, ax, r2 - row_lb2(G, cy, cz, ay, az, etol), etol, xl, xh);
            row_records(cell_start, row, xl, xh, rbeg, rlen);
        }
        // ---- sweep: the group's non-empty rows one after the other, 16 records at a time; survivors compacted into its LDS ----
        unsigned todo = (unsigned)(__ballot(rlen > 0) >> gbase) & 0xffffu;
        unsigned ns = 0;
        while (__any(todo != 0u)) {
            const bool has = todo != 0u;
            const int j = has ? __ffs((int)todo) - 1 : 0;
            todo &= todo - 1u;                                                  // (0 stays 0)
            const uint32_t vb = (uint32_t)__shfl((int)rbeg, gbase + j);
            const uint32_t vl = has ? (uint32_t)__shfl((int)rlen, gbase + j) : 0u;
            for (uint32_t o = 0; __any(o < vl); o += 16) {
                const bool ok = o + (uint32_t)gl < vl;
                const double4 P = rec[ok ? vb + o + (uint32_t)gl : 0u];
                const double dx = P.x - ax, dy = P.y - ay, dz = P.z - az;
                const double d2 = fma(dz, dz, fma(dy, dy, dx * dx));
                const bool sv = ok && d2 <= thr;
                const unsigned long long m = __ballot(sv);
                if (m) {
                    const unsigned mg = (unsigned)(m >> gbase) & 0xffffu;
                    const unsigned pos = ns + (unsigned)__popc(mg & ((1u << gl) - 1u));
                    if (sv && pos < (unsigned)KG_CAP) {
                        keys[pos].d2 = d2; keys[pos].idx = (uint32_t)__double_as_longlong(P.w); keys[pos].pad = vb + o + (uint32_t)gl;
                    }
                    ns += (unsigned)__popc(mg);
                }
                if (work) n_cand += ok ? 1 : 0;
            }
        }
        mine = mine && ns >= (unsigned)k && ns <= (unsigned)KG_CAP;
        if (active && !mine && gl == 0) {
            // not a one-pass case: the one-query-per-wave kernel does this slot in the next launch
            redo_list[atomicAdd(redo_count, 1u)] = (uint32_t)(slot0 + b);
        }
        if (work && gl == 0) { n_act += active ? 1 : 0; n_defer += (active && !mine) ? 1 : 0; n_surv += mine ? ns : 0; }
        // ---- rank by counting inside the group (entries gl, gl + 16, gl + 32, gl + 48), the four groups in lock step ----
        wave_lds_sync();
        const unsigned nsm = mine ? ns : 0u;
        unsigned nmax = nsm;
        { unsigned o = lane_xor32<16>(nmax); nmax = o > nmax ? o : nmax; o = lane_xor32<32>(nmax); nmax = o > nmax ? o : nmax; }
        nmax = (unsigned)__builtin_amdgcn_readfirstlane((int)nmax);
        double md[4]; uint32_t mi[4], mp[4]; unsigned rk[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const unsigned e = (unsigned)gl + 16u * t;
            const bool hs = e < nsm;
            md[t] = hs ? keys[e].d2 : __builtin_inf();
            mi[t] = hs ? keys[e].idx : 0xffffffffu;
            mp[t] = hs ? keys[e].pad : 0u;
            rk[t] = 0;
        }
        if (nmax <= 32u) {
            for (unsigned j = 0; j < nmax; ++j) {
                const double od = keys[j].d2; const uint32_t oi = keys[j].idx;      // (one address per group)
                const unsigned in = j < nsm ? 1u : 0u;
                rk[0] += in & (unsigned)((od < md[0]) | ((od == md[0]) & (oi < mi[0])));
                rk[1] += in & (unsigned)((od < md[1]) | ((od == md[1]) & (oi < mi[1])));
            }
        } else {
            for (unsigned j = 0; j < nmax; ++j) {
                const double od = keys[j].d2; const uint32_t oi = keys[j].idx;
                const unsigned in = j < nsm ? 1u : 0u;
#pragma unroll
                for (int t = 0; t < 4; ++t) rk[t] += in & (unsigned)((od < md[t]) | ((od == md[t]) & (oi < mi[t])));
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const unsigned e = (unsigned)gl + 16u * t;
            if (e < nsm && rk[t] < (unsigned)k) {
                const unsigned rr = rk[t];
                const double4 W = rec[mp[t]];
                nbr[3 * rr] = W.x; nbr[3 * rr + 1] = W.y; nbr[3 * rr + 2] = W.z;
                if (rr == (unsigned)(k - 1)) *dk_slot = md[t];
                if (idx_out) idx_out[q * k + rr] = idx_base + (int64_t)mi[t];
                if (d2_out) d2_out[q * k + rr] = md[t];
            }
        }
        wave_lds_sync();
        if (mine) dk_est = 0.75 * dk_est + 0.25 * *dk_slot;
        if (cov_out) {
            double mean = 0.0;
            if (gl < 3 && mine) {
                for (int s = 0; s < k; ++s) mean += nbr[3 * s + gl];
                mean /= (double)k;
            }
            const double m0 = __shfl(mean, gbase), m1 = __shfl(mean, gbase + 1), m2 = __shfl(mean, gbase + 2);
            if (gl < 6 && mine) {
                const int a = gl < 3 ? 0 : (gl < 5 ? 1 : 2);
                const int c = gl < 3 ? gl : (gl < 5 ? gl - 2 : 2);
                const double ma = a == 0 ? m0 : (a == 1 ? m1 : m2), mc = c == 0 ? m0 : (c == 1 ? m1 : m2);
                double cv = 0.0;
                for (int s = 0; s < k; ++s) cv = fma(nbr[3 * s + a] - ma, nbr[3 * s + c] - mc, cv);
                cov_out[6 * (slot0 + b) + gl] = cv * inv_km1;
            }
        }
        wave_lds_sync();
    }
    if (work) {
        n_cand = wsum_u64(n_cand); n_act = wsum_u64(n_act); n_defer = wsum_u64(n_defer); n_surv = wsum_u64(n_surv);
        if (lane == 0) { atomicAdd(work, n_cand); atomicAdd(work + 1, n_act - n_defer); atomicAdd(work + 3, n_surv); }
    }
