// sicp_tail_body.inc -- the body of the single-workgroup tail: included textually by k_icp_tail (sicp_tail.hip) and by the
// batched tail k_icp_tail_batch (one member per workgroup), so that both compile the same tokens (a shared __device__ function
// changed k_icp_tail's register allocation).  Names it uses: S (the kernel's LDS), st, dist, flag, p2, qx, qy, qz, normals, keep,
// resid, rec, A (TailArgs), the template parameter EPT, and the hand-over's PRE / tkt: PRE (a compile-time constant) = the next
// match may already be running and waits for this launch's ticket (DESIGN.md, "The tail -> match hand-over"): the loop state leaves
// through agent-scope stores, and EVERY exit stores A.seq in tkt[0] once all of the launch's device-memory writes are complete --
// after that only the record to pinned host memory follows.  tkt[PRE_ERR_WORD]: a waiting match gave up (the run stops, status 4).
    const int tid = threadIdx.x, wid = tid >> 6;
    const int Q = A.Q;
    long long tk[6]; tk[0] = clock64();
    // ---- loop state + this lane's correspondences: ONE global round trip (every load is issued before the first
    //      barrier and before the stop flag is looked at).  The rejection needs only the distances and verdicts -- 9 bytes per
    //      correspondence, asked for FIRST (loads return in order); the 60 bytes per correspondence the solver works on arrive
    //      while the order statistics are being taken ----
    double d[EPT];
    uint8_t fb[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        const int i = tid + e * TB;
        const int ic = i < Q ? i : Q - 1;                 // clamped: every lane loads, lanes past Q are masked below
        d[e] = dist[ic]; fb[e] = flag[ic];
    }
    double x[6], sc[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) { x[j] = st->x[j]; sc[j] = st->sc[j]; }
    const double w_state = st->w, prev_mean = st->prev_mean, prev_std = st->prev_std;
    const int done_iters = st->done_iters;
    int stop_in = st->stop;
    if constexpr (PRE) { if (tkt[PRE_ERR_WORD] != 0ull) stop_in = 2; }
    const int stop = stop_in;
    const double pmed = st->sel_med, pmad = st->sel_mad;               // the last launch's median and MAD (0: none) ...
    const int pcnt = st->sel_m;                                        // ... of this many distances
    Corr<EPT> C;
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        const int i = tid + e * TB;
        const int ic = i < Q ? i : Q - 1;
        C.px[e] = p2[3 * ic]; C.py[e] = p2[3 * ic + 1]; C.pz[e] = p2[3 * ic + 2];
        C.qx[e] = qx[ic]; C.qy[e] = qy[ic]; C.qz[e] = qz[ic];
        C.nx[e] = normals[3 * ic]; C.ny[e] = normals[3 * ic + 1]; C.nz[e] = normals[3 * ic + 2];
    }
    unsigned *hc = reinterpret_cast<unsigned *>(&S.ja[0][0]);      // the row staging area is idle until the LM phase
    for (int i = tid; i < HC * 257; i += TB) hc[i] = 0u;
    if (tid == 0) S.ncand = 0u;
    if (tid < 64) S.out[tid] = 0.0;
    if (stop) {
        // the run ended in an earlier launch (converged / failed): nothing to do but tell the host
        if constexpr (PRE) { if (tid == 0) publish_ticket(tkt, A.seq); }      // (this launch wrote nothing to device memory)
        if (tid == 0) __hip_atomic_store(rec + REC_STATUS, (PRE && stop == 2) ? 4.0 : 3.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (wid == 0) publish(rec, A.seq);
        return;
    }

    bool fl[EPT];
    unsigned long long key[EPT];
    unsigned nflag = 0;
    double dmn = __builtin_inf(), dmx = -__builtin_inf();
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        const int i = tid + e * TB;
        C.keep[e] = false; key[e] = NOKEY;
        fl[e] = i < Q && fb[e] != 0;
        if (i >= Q) d[e] = 0.0;
        if (fl[e]) { key[e] = okey(d[e]); dmn = fmin(dmn, d[e]); dmx = fmax(dmx, d[e]); }
        nflag += (unsigned)__popcll((long long)__ballot(fl[e]));
    }
    // a settled run: both statistics are looked for in a window around the last launch's first (window_collect).  Half widths in
    // units of the MAD, sized for ~40 of the `pcnt` keys (a normal density holds 0.27 n keys per MAD at its median, 0.43 n of the
    // absolute deviations at theirs)
    bool win = A.window != 0 && pmad > 0.0 && pmad < __builtin_inf() && pcnt > 0;
    const double hw_med = pmad * fmin(0.25, 75.0 / (double)pcnt), hw_mad = pmad * fmin(0.25, 47.0 / (double)pcnt);
    if (win) window_collect<EPT>(S, 0, key, okey(pmed - hw_med), okey(pmed + hw_med));
    // survivors of the planarity test: wave counts + one barrier.  The RANGE of their distances (two wave reductions, the histogram
    // selection's first interval) is only formed when that selection runs: a settled run reads both statistics off its windows
    bool have_range = !win;
    if (have_range) { dmn = wmin_f64(dmn); dmx = wmin_f64(-dmx); }
    if ((tid & 63) == 0) { S.wcnt[wid] = nflag; if (have_range) { S.dmm[wid][0] = dmn; S.dmm[wid][1] = dmx; } }
    __syncthreads();
    long m = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) m += S.wcnt[w];
    if (have_range) {
#pragma unroll
        for (int w = 0; w < NW; ++w) { dmn = fmin(dmn, S.dmm[w][0]); dmx = fmin(dmx, S.dmm[w][1]); }
    }
    tk[1] = clock64();

    if (m == 0) {
#pragma unroll
        for (int e = 0; e < EPT; ++e) { const int i = tid + e * TB; if (i < Q) { keep[i] = 0; resid[i] = 0.0; } }
        if (tid == 0) {
            S.out[1] = __builtin_nan(""); S.out[2] = __builtin_nan("");
            for (int k = 0; k < 6; ++k) S.out[10 + k] = x[k];
            S.out[REC_STATUS] = 1.0;
            if constexpr (!PRE) st->stop = 1;
        }
        if constexpr (PRE) {
            drain_block();                    // keep mask and residuals of all four waves are written
            if (tid == 0) { store_stop(st); publish_ticket(tkt, A.seq); }
        }
        if (wid == 0) { flush_rec(S, rec, REC_TICKET); publish(rec, A.seq); }
        return;
    }

    // ---- median / raw MAD (corrpts.py:165-188): np.median = mean of the two middle values ----
    double med = 0.0, mad = 0.0;
    int rounds[2] = {0, 0};
    long long tsel = 0;
#pragma unroll 1
    for (int which = 0; which < 2; ++which) {
        if (which == 1) {
#pragma unroll
            for (int e = 0; e < EPT; ++e) if (fl[e]) key[e] = okey(fabs(d[e] - med));
            tsel = clock64();
            if (win) {
                window_collect<EPT>(S, 1, key, okey(fmax(pmad - hw_mad, 0.0)), okey(pmad + hw_mad));
                __syncthreads();
            }
        }
        unsigned long long ka, kb;
        int nr = 0;
#ifdef SICP_SEL_FINE_TRACE
        if (tid == 0) S.selw = which;
        __syncthreads();
#endif
        // (one miss ends the attempts of this launch: a median that moved takes the MAD with it)
        if (win) win = window_pick(S, which, (m - 1) / 2, (m & 1) == 0, ka, kb);
        if (!win) {
            if (!have_range) {
                // the window missed: the distances' range after all (dmn / dmx still hold this lane's own: d is untouched)
                dmn = wmin_f64(dmn); dmx = wmin_f64(-dmx);
                if ((tid & 63) == 0) { S.dmm[wid][0] = dmn; S.dmm[wid][1] = dmx; }
                __syncthreads();
#pragma unroll
                for (int w = 0; w < NW; ++w) { dmn = fmin(dmn, S.dmm[w][0]); dmx = fmin(dmx, S.dmm[w][1]); }
                have_range = true;
            }
            // the interval that holds every key: the distances' own, or (|d - med| is monotone in d on either side of med) what follows from it
            unsigned long long klo = okey(dmn), khi = okey(-dmx);
            if (which == 1) { const double u = fabs(dmn - med), v = fabs(-dmx - med); klo = okey(0.0); khi = okey(u > v ? u : v); }
            block_select<EPT>(S, hc, key, (m - 1) / 2, (m & 1) == 0, klo, khi, ka, kb, nr);
        }
        const double mid = (oval(ka) + oval(kb)) / 2.0;
        if (which == 0) { med = mid; rounds[0] = nr; } else { mad = mid; rounds[1] = nr; }
    }
    const double bound = 3 * mad;
    tk[2] = clock64();

    // ---- keep mask.  The kept distances' count / mean / std (simpleicp.py:233-234) are only needed NOW when the
    //      weight is still automatic (first iteration of such a run): then one pass over deviations from the median
    //      (a shift within a few MAD of the mean: var = (S2 - S1^2 / n) / n loses nothing to cancellation).  Otherwise
    //      they come for free out of the first evaluation's Gram matrix below (r = d at the start estimate). ----
    const bool need_w = !(w_state > 0);
    double v3[3] = {0.0, 0.0, 0.0};
    unsigned nkeep = 0;
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        const int i = tid + e * TB;
        const double dev = d[e] - med;
        const bool kq = fl[e] && fabs(dev) <= bound;
        C.keep[e] = kq;
        if (i < Q) keep[i] = kq ? 1 : 0;
        if (kq) { v3[0] += 1.0; v3[1] += dev; v3[2] = fma(dev, dev, v3[2]); }
        nkeep += (unsigned)__popcll((long long)__ballot(kq));
    }
    double nk, dmean = 0.0, dstd = 0.0;
    if (need_w) {
        block_sum<3>(v3, S.red[0]);
        nk = v3[0]; dmean = med + v3[1] / nk;
        const double dvar = (v3[2] - v3[1] * v3[1] / nk) / nk;
        dstd = sqrt(dvar > 0.0 ? dvar : 0.0);
    } else {
        if ((tid & 63) == 0) S.wcnt[wid] = nkeep;        // (its earlier content was consumed two barriers ago)
        __syncthreads();
        unsigned nkw = (S.wcnt[0] + S.wcnt[1]) + (S.wcnt[2] + S.wcnt[3]);
        if constexpr (NW == 8) nkw += (S.wcnt[4] + S.wcnt[5]) + (S.wcnt[6] + S.wcnt[7]);
        nk = (double)nkw;
    }
    if (tid == 0) { S.out[0] = (double)m; S.out[1] = med; S.out[2] = mad; S.out[3] = nk; S.out[4] = dmean; S.out[5] = dstd; }
    if (nk < 6.0) {
#pragma unroll
        for (int e = 0; e < EPT; ++e) { const int i = tid + e * TB; if (i < Q) resid[i] = 0.0; }
        if (tid == 0) {
            for (int k = 0; k < 6; ++k) S.out[10 + k] = x[k];
            S.out[REC_STATUS] = 1.0;
            if constexpr (!PRE) st->stop = 1;
        }
        if constexpr (PRE) {
            drain_block();                    // keep mask and residuals of all four waves are written
            if (tid == 0) { store_stop(st); publish_ticket(tkt, A.seq); }
        }
        if (wid == 0) { flush_rec(S, rec, REC_TICKET); publish(rec, A.seq); }
        return;
    }
    const double w = need_w ? 1.0 / (dstd * dstd) : w_state;          // simpleicp.py:233-234 (frozen afterwards)
    tk[3] = clock64();

    // ---- Levenberg-Marquardt on the fused 6x6 reductions (same acceptance rules as the host solver);
    //      one evaluation site: the first evaluation is a trial that is always accepted ----
    int nfree = 0;
#pragma unroll
    for (int j = 0; j < 6; ++j) nfree += (A.ow[j] < __builtin_inf()) ? 1 : 0;
    double xn[6], scn[6], rr[EPT], rrn[EPT];
#pragma unroll
    for (int j = 0; j < 6; ++j) { xn[j] = x[j]; scn[j] = sc[j]; }
    int steps = 0, evals = 0, cur = 1, tries = 0;
    bool first = true;
    double d0n = 1.0, d0s1 = 0.0, d0s2 = 0.0;
    double cost = 0.0, lambda = 0.0, dxmax = 0.0;
    // finer split of the solver loop (-DSICP_TAIL_FINE_TRACE: each reading drains the LDS queue, ~100 cycles -- off by default;
    // measured at C4: evaluation 5.35 k cycles, acceptance 1.05 k, 6x6 solve 2.3 k, trial angles + loop 2.2 k per round)
#ifdef SICP_TAIL_FINE_TRACE
#define SICP_FT(x) x
#else
#define SICP_FT(x)
#endif
    long long t_eval = 0, t_step = 0, t_acc = 0;
#pragma unroll 1
    for (;;) {
        SICP_FT(const long long te0 = clock64();)
#ifdef SICP_TAIL_MFMA_GRAM
        eval_ne_mfma<EPT>(S, xn, scn, C, rrn, cur ^ 1); ++evals;      // (its first barrier orders it after the last one's LDS reads)
#else
        eval_ne<EPT>(S, xn, scn, C, rrn, cur ^ 1, evals & 1); ++evals;
#endif
        SICP_FT(const long long te1 = clock64(); t_eval += te1 - te0;)
        const double costn = objective(S.gf[wid][cur ^ 1], w, xn, A);
        if (first) {
            // r = d at the start estimate: sum r, sum r^2, n of this evaluation ARE the kept distances' statistics (turned into
            // mean / std where the record is written: two divisions and a root are not on the solver's path)
            const double *G0 = S.gf[wid][cur ^ 1];
            d0n = G0[7 * 8 + 7]; d0s1 = G0[6 * 8 + 7]; d0s2 = G0[6 * 8 + 6];
        }
        if (first || costn <= cost * (1 + 1e-12) || dxmax < 1e-15) {          // 1e-12: rounding noise of the sums
#pragma unroll
            for (int j = 0; j < 6; ++j) { x[j] = xn[j]; sc[j] = scn[j]; }
#pragma unroll
            for (int e = 0; e < EPT; ++e) rr[e] = rrn[e];
            cur ^= 1; cost = costn; tries = 0;
            if (!first) {
                lambda = lambda > 0 ? lambda * 0.1 : 0.0;
                if (lambda < 1e-12) lambda = 0.0;
                ++steps;
                double xmax = 0.0;
#pragma unroll
                for (int j = 0; j < 6; ++j) xmax = fmax(xmax, fabs(x[j]));
                if (dxmax <= 1e-13 * (1.0 + xmax)) break;
            }
            first = false;
            if (steps >= A.max_steps || nfree == 0) break;
        } else {
            lambda = lambda > 0 ? lambda * 10 : 1e-6;
            if (++tries >= 40) break;
        }
        // next trial from (x, lambda)
        bool ok = false;
        double dstep[6];
        SICP_FT(const long long ts0 = clock64(); t_acc += ts0 - te1;)
#pragma unroll 1
        for (; tries < 40; ++tries) {
            ok = lm_step(S.gf[wid][cur], w, x, lambda, A, dstep);
            dxmax = 0.0;
#pragma unroll
            for (int j = 0; j < 6; ++j) { xn[j] = x[j] + dstep[j]; dxmax = fmax(dxmax, fabs(dstep[j])); }
            ok = ok && (dxmax < __builtin_inf());
            if (ok) break;
            lambda = lambda > 0 ? lambda * 10 : 1e-6;
        }
        SICP_FT(t_step += clock64() - ts0;)
        if (!ok) break;
        double xm = 0.0;
#pragma unroll
        for (int j = 0; j < 6; ++j) xm = fmax(xm, fabs(x[j]));
        // the undamped Gauss-Newton step from x is below 1e-10: x is the minimiser to that accuracy (the reference stops at 1e-8)
        if (lambda == 0.0 && dxmax <= 1e-10 * (1.0 + xm)) break;
#pragma unroll
        for (int j = 0; j < 3; ++j) sincos_step(xn[j], dstep[j], sc[2 * j], sc[2 * j + 1], scn[2 * j], scn[2 * j + 1]);
    }
    tk[4] = clock64();

    // ---- residuals at the optimum (rr belongs to x: rejected trials only wrote rrn); their mean / std (ddof 0) come
    //      out of the accepted evaluation's Gram matrix: sum r, sum r^2, n (at the optimum |mean| is well below std, so
    //      sum r^2 / n - mean^2 keeps its digits) ----
    const double *G = S.gf[wid][cur];
    const double gn = G[7 * 8 + 7];
    const double rmean = G[6 * 8 + 7] / gn;
    const double rvar = G[6 * 8 + 6] / gn - rmean * rmean;
    const double rstd = sqrt(rvar > 0.0 ? rvar : 0.0);
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        const int i = tid + e * TB;
        if (i < Q) resid[i] = rr[e];
    }
    const bool finite = cost < __builtin_inf();
    // convergence test of simpleicp.py:356-379 on (mean, std) of this and the previous iteration's residuals
    bool conv = false;
    if (A.min_change >= 0.0 && done_iters > 0 && finite) {
        const double cm = prev_mean == 0.0 ? (rmean == 0.0 ? 0.0 : __builtin_inf()) : fabs((rmean - prev_mean) / prev_mean * 100.0);
        const double cs = prev_std == 0.0 ? (rstd == 0.0 ? 0.0 : __builtin_inf()) : fabs((rstd - prev_std) / prev_std * 100.0);
        conv = cm < A.min_change && cs < A.min_change;
    }
    if constexpr (!PRE) { if (wid > 1) return; }
    if (wid == 1) {
        // ---- wave 1: the next iteration's start (estimate, its sin / cos, H(x) and the rigid inverse [R^T | -R^T t]) leaves as one
        //      store -- while wave 0 assembles and publishes the record (every lane of every wave holds the same estimate) ----
        if (tid == 64) {
            IcpDev n;
            double Hn[12];
            euler_H(x, sc, Hn);
#pragma unroll
            for (int j = 0; j < 6; ++j) { n.x[j] = x[j]; n.sc[j] = sc[j]; }
#pragma unroll
            for (int j = 0; j < 12; ++j) n.H.m[j] = Hn[j];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int j = 0; j < 3; ++j) n.Hinv.m[4 * i + j] = Hn[4 * j + i];
                n.Hinv.m[4 * i + 3] = -(Hn[i] * Hn[3] + Hn[4 + i] * Hn[7] + Hn[8 + i] * Hn[11]);
            }
            n.w = w; n.prev_mean = rmean; n.prev_std = rstd;
            n.done_iters = done_iters + 1; n.stop = (conv || !finite) ? 1 : 0; n.sel_m = (int)m; n.pad = 0;
            n.sel_med = med; n.sel_mad = mad;
            const double *src = reinterpret_cast<const double *>(&n);
#pragma unroll
            for (int j = 0; j < ST_DOUBLES; ++j) S.out2[j] = src[j];
        }
        flush_state<PRE>(S, reinterpret_cast<double *>(st), ST_DOUBLES);
        if constexpr (!PRE) return;
    }
    if constexpr (PRE) {
        // the hand-over: residuals and keep mask of all four waves and the new loop state are complete (each wave drains its own
        // stores, then the barrier), wave 1 publishes the ticket -- the waiting match starts -- while wave 0 assembles the record
        drain_block();
        if (tid == 64) publish_ticket(tkt, A.seq);
        if (wid != 0) return;
    }
    // ---- wave 0: the record (pinned host memory) ----
    if (tid < 30) {
        // record layout of the 30 sums: 21 upper-triangle entries of J^T J (row-major), 6 of J^T r, sum r, sum r^2, n
        int u = 0, v = 0;
        if (tid < 21) { int t = tid; while (t >= 6 - u) { t -= 6 - u; ++u; } v = u + t; }
        else if (tid < 27) { u = tid - 21; v = 6; }
        else if (tid == 27) { u = 6; v = 7; }
        else if (tid == 28) { u = 6; v = 6; }
        else { u = 7; v = 7; }
        S.out[20 + tid] = G[u * 8 + v];
    }
    if (tid == 0) {
        if (!need_w) {
            const double mean0 = d0s1 / d0n, var0 = d0s2 / d0n - mean0 * mean0;
            S.out[4] = mean0; S.out[5] = sqrt(var0 > 0.0 ? var0 : 0.0);
        }
        S.out[6] = w; S.out[7] = cost; S.out[8] = steps; S.out[9] = evals;
#pragma unroll
        for (int j = 0; j < 6; ++j) S.out[10 + j] = x[j];
        S.out[16] = rmean; S.out[17] = rstd;
        S.out[REC_STATUS] = finite ? 0.0 : 2.0;
        S.out[REC_CONVERGED] = conv ? 1.0 : 0.0;
        tk[5] = clock64();
#pragma unroll
        for (int k = 0; k < 5; ++k) S.out[50 + k] = (double)(tk[k + 1] - tk[k]);
        S.out[59] = (double)t_eval; S.out[60] = (double)t_step; S.out[62] = (double)t_acc;
        S.out[55] = (double)(tsel - tk[1]); S.out[56] = rounds[0]; S.out[57] = (double)(tk[2] - tsel); S.out[58] = rounds[1];
#ifdef SICP_EVAL_FINE_TRACE
        for (int i = 0; i < 5; ++i) S.out[38 + i] = (double)(S.evt[i + 1] - S.evt[i]);
#endif
#ifdef SICP_SEL_FINE_TRACE
        // (trace build: the splits of both selections overwrite the last twelve normal-equation sums of the record)
        for (int wsel = 0; wsel < 2; ++wsel)
            for (int i = 0; i < 6; ++i) S.out[38 + 6 * wsel + i] = (double)(S.selt[wsel][i + 1] - S.selt[wsel][i]);
#endif

    }
    flush_rec(S, rec, REC_TICKET);
    publish(rec, A.seq);
