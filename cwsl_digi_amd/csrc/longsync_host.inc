// longsync_host.inc -- host glue of the 120 s modes' candidate search (included by cwsl_gpu.hip).  See longsync_kernels.hpp for
// the algorithms and their "parity unpinned" status; every table here is built exactly as oracle/longsync_oracle.c builds its own.
namespace {

std::vector<float2> fftb_table(int n)
{
    constexpr double pi = 3.14159265358979323846;
    std::vector<float2> t((size_t)n);
    for (int k = 0; k < n; ++k) t[k] = make_float2((float)std::cos(2.0 * pi * k / n), (float)(-std::sin(2.0 * pi * k / n)));
    t[0] = make_float2(1.f, 0.f);
    return t;
}

int long_upload(cwslg_ctx *c, const std::vector<float2> &h, float2 **d)
{
    HIPCHK(c, hipMalloc((void **)d, h.size() * sizeof(float2)));
    HIPCHK(c, hipMemcpy(*d, h.data(), h.size() * sizeof(float2), hipMemcpyHostToDevice));
    return CWSLG_OK;
}

int long_ensure_fftb(cwslg_ctx *c, LongShared::Plan &p, int na, int nb)
{
    if (p.wa) return CWSLG_OK;
    int rc;
    const std::vector<float2> wa = fftb_table(na);
    if ((rc = long_upload(c, wa, &p.wa)) != CWSLG_OK) return rc;
    std::vector<float2> full((size_t)na * na);             // stage 1's matrix: full[c][a] = WA[(a c) mod NA]
    for (int cc = 0; cc < na; ++cc)
        for (int a = 0; a < na; ++a) full[(size_t)cc * na + a] = wa[(size_t)((a * cc) % na)];
    if ((rc = long_upload(c, full, &p.wfull)) != CWSLG_OK) return rc;
    {   // the twiddle between the stages, W_N^(b c), laid out [c][b] (round 4): a wave's 64 columns b of one output c are ONE 512-byte run.  The flat table
        // indexed b * c made every lane of that read touch its own cache line (stride 8 c bytes): 184 KB through the L2 per 23 KB tile.
        const std::vector<float2> wn = fftb_table(na * nb);
        std::vector<float2> wnt((size_t)na * nb);
        for (int cc = 0; cc < na; ++cc)
            for (int b = 0; b < nb; ++b) wnt[(size_t)cc * nb + b] = wn[(size_t)b * cc];
        if ((rc = long_upload(c, wnt, &p.wn)) != CWSLG_OK) return rc;
    }
    std::vector<float2> wb = fftb_table(nb);
    wb.resize((size_t)nb / 2);
    wb[(size_t)nb / 4] = make_float2(0.f, -1.f);
    return long_upload(c, wb, &p.wb);
}

int long_ensure_wspr_tables(cwslg_ctx *c)
{
    LongShared &s = c->long_shared;
    int rc = long_ensure_fftb(c, s.p45, 45, 1024);
    if (rc || s.d_wspr_T) return rc;
    constexpr double pi = 3.14159265358979323846;
    {   // T_a[i] = exp(-2 pi i a j_i / nfft1), j_i = i0 + i (- 46080 above the middle), i0 = 184320 (1500 Hz)
        std::vector<float2> T((size_t)WSPR_R * WSPR_M);
        const double df = 12000.0 / WSPR_NFFT1;
        const long i0 = (long)(1500.0 / df + 0.5);
        for (int a = 0; a < WSPR_R; ++a)
            for (int i = 0; i < WSPR_M; ++i) {
                long j = i0 + i;
                if (i > WSPR_M / 2) j -= WSPR_M;
                const long ph = ((long)a * j) % WSPR_NFFT1;
                const double ang = 2.0 * pi * (double)ph / (double)WSPR_NFFT1;
                // stored in the combine kernel's access order: T[a][c][d] with i = c + 45 d
                T[(size_t)a * WSPR_M + (size_t)(i % 45) * 1024 + i / 45] =
                    (ph == 0) ? make_float2(1.f, 0.f) : make_float2((float)std::cos(ang), (float)(-std::sin(ang)));
            }
        if ((rc = long_upload(c, T, &s.d_wspr_T)) != CWSLG_OK) return rc;
    }
    {
        std::vector<float2> w512 = fftb_table(512);
        w512.resize(256);
        w512[128] = make_float2(0.f, -1.f);
        if ((rc = long_upload(c, w512, &s.d_w512)) != CWSLG_OK) return rc;
        std::vector<float> win(512);
        for (int j = 0; j < 512; ++j) win[j] = (float)std::sin(0.006147931 * (double)j);
        HIPCHK(c, hipMalloc((void **)&s.d_win512, win.size() * sizeof(float)));
        HIPCHK(c, hipMemcpy(s.d_win512, win.data(), win.size() * sizeof(float), hipMemcpyHostToDevice));
        static const unsigned char pr3[162] = {
            1,1,0,0,0,0,0,0,1,0,0,0,1,1,1,0,0,0,1,0, 0,1,0,1,1,1,1,0,0,0,0,0,0,0,1,0,0,1,0,1,
            0,0,0,0,0,0,1,0,1,1,0,0,1,1,0,1,0,0,0,1, 1,0,1,0,0,0,0,1,1,0,1,0,1,0,1,0,1,0,0,1,
            0,0,1,0,1,1,0,0,0,1,1,0,1,0,1,0,0,0,1,0, 0,0,0,0,1,0,0,1,0,0,1,1,1,0,1,1,0,0,1,1,
            0,1,0,0,0,1,1,1,0,0,0,0,0,1,0,1,0,0,1,1, 0,0,0,0,0,0,0,1,1,0,1,0,1,1,0,0,0,1,1,0,
            0,0};
        HIPCHK(c, hipMalloc((void **)&s.d_pr3, sizeof(pr3)));
        HIPCHK(c, hipMemcpy(s.d_pr3, pr3, sizeof(pr3), hipMemcpyHostToDevice));
    }
    return CWSLG_OK;
}

// get_candidates_fst4's derived integers for the configured window (float arithmetic as in the restatement)
int long_fst4w_params(const LongConfig &cfg, Fst4wParams *P, int *nband)
{
    const float fs = 12000.0f;
    const float df1 = fs / (float)F4W_NMAX, baud = fs / (float)F4W_NSPS, df2 = baud / 2.0f;
    const int nd = (int)(df2 / df1), ndh = nd / 2;
    const int ia = (int)std::lround(std::fmax(100.0f, (float)cfg.nfa_hz) / df2), ib = (int)std::lround(std::fmin(4800.0f, (float)cfg.nfb_hz) / df2);
    const int ina = ia, inb = ib;                           // signal window == noise window (-L/-H of the reference's command)
    const int nnw = (int)std::lround(48000.0f * (float)F4W_NSPS * 2.0f / fs);
    if (inb < ina || inb >= nnw || nnw > F4W_NNW) return CWSLG_ERR_ARG;
    const int jlo = (int)std::lround((float)ina * df2 / df1) - ndh, jhi = (int)std::lround((float)inb * df2 / df1) + ndh;
    if (jlo < 0 || jhi > F4W_NMAX / 2 || jhi - jlo + 1 > F4W_M || inb - ina + 9 > 1024) return CWSLG_ERR_ARG;
    // what the band kernel's table holds: F4W_TP entries per residue mod 125, and dlo(c) computed for jlo > 125 (the 100 Hz clamp keeps
    // jlo at 11986 and above, so only the first limit is reachable: 1400..1607 is the widest window above 1400 Hz, nband 24936)
    if ((jhi - jlo + 1 + 124) / 125 > F4W_TP || jlo <= 125) return CWSLG_ERR_ARG;
    P->ina = ina; P->inb = inb; P->ia = ia; P->ib = ib; P->ndh = ndh; P->jlo = jlo; P->nnw = nnw;
    P->df1 = df1; P->df2 = df2; P->minsync = cfg.minsync;
    *nband = jhi - jlo + 1;
    return CWSLG_OK;
}

int long_ensure_fst4w_tables(cwslg_ctx *c)
{
    LongShared &s = c->long_shared;
    int rc = long_ensure_fftb(c, s.p125, 125, 256);
    if (rc) return rc;
    Fst4wParams P; int nband = 0;
    if ((rc = long_fst4w_params(c->long_cfg, &P, &nband)) != CWSLG_OK) return fail(c, rc, "FST4W search window out of range");
    if ((nband + 124) / 125 > F4W_TP || P.jlo <= 125) return fail(c, CWSLG_ERR_ARG, "FST4W search window out of range");   // guard: long_fst4w_params rejects these
    if (s.d_f4w_T && s.f4w_jlo == P.jlo && s.f4w_nband == nband) return CWSLG_OK;
    if (s.d_f4w_T) { HIPCHK(c, sync_streams(c)); (void)hipFree(s.d_f4w_T); s.d_f4w_T = nullptr; }
    constexpr double pi = 3.14159265358979323846;
    // stored in the band kernel's access order: T[a][c][t], k = c + 125 (dlo(c) + t)
    std::vector<float2> T((size_t)F4W_R * 125 * F4W_TP, make_float2(0.f, 0.f));
    for (int cc = 0; cc < 125; ++cc) {
        const int dlo = (P.jlo - cc + 124) / 125;
        for (int t = 0; t < F4W_TP; ++t) {
            const long k = cc + 125L * (dlo + t);
            if (k >= P.jlo + nband) break;
            for (int a = 0; a < F4W_R; ++a) {
                const long ph = ((long)a * k) % F4W_NMAX;
                const double ang = 2.0 * pi * (double)ph / (double)F4W_NMAX;
                T[((size_t)a * 125 + cc) * F4W_TP + t] = (ph == 0) ? make_float2(1.f, 0.f) : make_float2((float)std::cos(ang), (float)(-std::sin(ang)));
            }
        }
    }
    if ((rc = long_upload(c, T, &s.d_f4w_T)) != CWSLG_OK) return rc;
    s.f4w_jlo = P.jlo; s.f4w_nband = nband;
    return CWSLG_OK;
}

int long_ensure_channel(cwslg_ctx *c, Channel &ch)
{
    LongChannelBuffers &b = ch.longbuf;
    if (b.d_block) return CWSLG_OK;
    auto up = [](size_t v) { return (v + 255) & ~size_t(255); };
    const bool wspr = ch.sync_wspr;
    const size_t z = up((size_t)(wspr ? 16 * WSPR_M : 23 * F4W_M) * sizeof(float2));
    const size_t aux = up((size_t)(wspr ? 2 * WSPR_M : F4W_M) * sizeof(float2));
    const size_t iq = wspr ? up((size_t)WSPR_IQ_LEN * sizeof(float2)) : 0;
    const size_t ps = wspr ? up((size_t)WSPR_NFFTS * 512 * sizeof(float)) : 0;
    const size_t vec = up((size_t)(wspr ? 416 : F4W_NNW) * sizeof(float));
    const size_t cand = up(wspr ? WSPR_MAXCAND * sizeof(WsprCand) : F4W_MAXCAND * sizeof(Fst4wCand));
    HIPCHK(c, hipMalloc((void **)&b.d_block, 2 * z + aux + iq + 2 * ps + vec + cand + 256));
    char *p = b.d_block;
    b.w.z = (float2 *)p; p += z;
    b.w.y = (float2 *)p; p += z;
    b.w.aux = (float2 *)p; p += aux;
    b.w.iq = (float2 *)p; p += iq;
    b.w.ps = (float *)p; p += ps;
    b.w.sq = (float *)p; p += ps;
    b.w.vec = (float *)p; p += vec;
    b.w.cand = p; p += cand;
    b.w.ncand = (int *)p;
    b.w.frame = ch.d_i16;
    b.w.frame_len = (int)ch.frame_len;
    HIPCHK(c, hipMemsetAsync(b.w.ncand, 0, 256, c->stream));
    return CWSLG_OK;
}

// Candidate search on the frames finalised by this boundary: WSPR channels through wsprd's front end, FST4W-120 channels through
// get_candidates_fst4.  One batched launch per stage over all channels of a mode.
int long_sync_launch(cwslg_ctx *c, const std::vector<int> &emitted)
{
    std::vector<LongWork> ww, wf;
    for (int id : emitted) {
        Channel &ch = c->chans[id];
        if (!ch.sync_wspr && !ch.sync_fst4w) continue;
        int rc = long_ensure_channel(c, ch);
        if (rc) return rc;
        (ch.sync_wspr ? ww : wf).push_back(ch.longbuf.w);
        ch.stamp[REC_CAND] = ch.frame_t0;       // the list now queued belongs to this frame
    }
    if (ww.empty() && wf.empty()) return CWSLG_OK;
    int rc;
    if (!ww.empty() && (rc = long_ensure_wspr_tables(c)) != CWSLG_OK) return rc;
    if (!wf.empty() && (rc = long_ensure_fst4w_tables(c)) != CWSLG_OK) return rc;
    const size_t nw = ww.size(), nf = wf.size();
    WorkBuf *wb = acquire_workbuf(c, (nw + nf) * sizeof(LongWork));
    if (!wb) return fail(c, CWSLG_ERR_NOMEM, "work buffer allocation failed");
    if (nw) std::memcpy(wb->h, ww.data(), nw * sizeof(LongWork));
    if (nf) std::memcpy((LongWork *)wb->h + nw, wf.data(), nf * sizeof(LongWork));
    HIPCHK(c, upload_workbuf(c, wb, (nw + nf) * sizeof(LongWork)));
    hipEvent_t ea, eb;
    span_begin(c, 2, &ea, &eb);
    const LongShared &s = c->long_shared;
    if (nw) {
        const LongWork *d = (const LongWork *)wb->d;
        const FftbTables tb{s.p45.wa, s.p45.wn, s.p45.wb, s.p45.wfull};
        const unsigned n = (unsigned)nw;
        hipLaunchKernelGGL(wspr_pack_kernel, dim3(WSPR_M / 256, n), dim3(256), 0, c->stream, d);
        // 45 x 1024: the VALU form is the faster one (0.63 against 1.14 ms per 128 frames: a 45-row product wastes 30 % of two 32-row
        // matrix tiles); CWSLG_LONG_VARIANT bit 1 selects the matrix-core form (same bits)
#if CWSLG_LAB
        const bool valu1 = (c->long_variant & 2) == 0;
        if (!valu1) hipLaunchKernelGGL((fftb_stage1_mfma_kernel<45, 1024>), dim3(1024 / 32, 16, n), dim3(128), 0, c->stream, d, tb, 0, 0);
        else
#endif
        hipLaunchKernelGGL((fftb_stage1_kernel<45, 1024>), dim3(1024 / 64, 16, n), dim3(FFTB_S1_NT), 0, c->stream, d, tb, tb.wfull, 0, 0);
        hipLaunchKernelGGL((fftb_stage2_kernel<45, 1024>), dim3((45 + 3) / 4, 16, n), dim3(256), 0, c->stream, d, tb, 0);
        hipLaunchKernelGGL(wspr_combine_kernel, dim3(45, n), dim3(256), 0, c->stream, d, (const float2 *)s.d_wspr_T);
#if CWSLG_LAB
        if (!valu1) hipLaunchKernelGGL((fftb_stage1_mfma_kernel<45, 1024>), dim3(1024 / 32, 1, n), dim3(128), 0, c->stream, d, tb, 1, 1);
        else
#endif
        hipLaunchKernelGGL((fftb_stage1_kernel<45, 1024>), dim3(1024 / 64, 1, n), dim3(FFTB_S1_NT), 0, c->stream, d, tb, tb.wfull, 1, 1);
        hipLaunchKernelGGL((fftb_stage2_kernel<45, 1024>), dim3((45 + 3) / 4, 1, n), dim3(256), 0, c->stream, d, tb, 1);
        hipLaunchKernelGGL(wspr_iq_kernel, dim3((WSPR_IQ_LEN + 255) / 256, n), dim3(256), 0, c->stream, d);
        hipLaunchKernelGGL(wspr_spectra_kernel, dim3(WSPR_NFFTS, n), dim3(256), 0, c->stream, d, (const float2 *)s.d_w512, (const float *)s.d_win512);
        hipLaunchKernelGGL(wspr_peaks_kernel, dim3(n), dim3(512), 0, c->stream, d);
        hipLaunchKernelGGL(wspr_coarse_kernel, dim3(WSPR_MAXCAND, n), dim3(256), 0, c->stream, d, (const unsigned char *)s.d_pr3);
    }
    if (nf) {
        const LongWork *d = (const LongWork *)wb->d + nw;
        const FftbTables tb{s.p125.wa, s.p125.wn, s.p125.wb, s.p125.wfull};
        const unsigned n = (unsigned)nf;
        Fst4wParams P; int nband = 0;
        (void)long_fst4w_params(c->long_cfg, &P, &nband);
        hipLaunchKernelGGL(fst4w_pack_kernel, dim3(F4W_M / 256, n), dim3(256), 0, c->stream, d);
#if CWSLG_LAB
        if (c->long_variant & 1) hipLaunchKernelGGL((fftb_stage1_kernel<125, 256>), dim3(256 / 64, 23, n), dim3(FFTB_S1_NT), 0, c->stream, d, tb, tb.wfull, 0, 0);
        else
#endif
        hipLaunchKernelGGL((fftb_stage1_mfma_kernel<125, 256>), dim3(256 / 32, 23, n), dim3(256), 0, c->stream, d, tb, 0, 0);
        hipLaunchKernelGGL((fftb_stage2_kernel<125, 256>), dim3((125 + 15) / 16, 23, n), dim3(256), 0, c->stream, d, tb, 0);
        hipLaunchKernelGGL(fst4w_band_kernel, dim3(125, n), dim3(256), 0, c->stream, d, (const float2 *)s.d_f4w_T, P.jlo, nband);
        hipLaunchKernelGGL(fst4w_cand_kernel, dim3(n), dim3(512), 0, c->stream, d, P);
    }
    span_end(c, eb);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(wb->done, c->stream));
    wb->in_flight = true;
    c->stats.sync_launches++;
    return CWSLG_OK;
}

void long_free_shared(LongShared &s)
{
    for (LongShared::Plan *p : {&s.p45, &s.p125}) {
        if (p->wa) (void)hipFree(p->wa);
        if (p->wn) (void)hipFree(p->wn);
        if (p->wb) (void)hipFree(p->wb);
        if (p->wfull) (void)hipFree(p->wfull);
    }
    if (s.d_wspr_T) (void)hipFree(s.d_wspr_T);
    if (s.d_f4w_T) (void)hipFree(s.d_f4w_T);
    if (s.d_w512) (void)hipFree(s.d_w512);
    if (s.d_win512) (void)hipFree(s.d_win512);
    if (s.d_pr3) (void)hipFree(s.d_pr3);
    s = LongShared();
}

} // namespace

extern "C" {

int cwslg_enable_long_sync(cwslg_ctx *c, int enable, int fst4w_nfa_hz, int fst4w_nfb_hz, float fst4w_minsync)
{
    if (!c) return CWSLG_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    if (!enable) { c->long_cfg.enabled = false; return CWSLG_OK; }
    LongConfig cfg;
    cfg.enabled = true; cfg.nfa_hz = fst4w_nfa_hz; cfg.nfb_hz = fst4w_nfb_hz; cfg.minsync = fst4w_minsync;
    Fst4wParams P; int nband = 0;
    if (long_fst4w_params(cfg, &P, &nband) != CWSLG_OK) return fail(c, CWSLG_ERR_ARG, "FST4W search window out of range");
    c->long_cfg = cfg;
    return CWSLG_OK;
}

int cwslg_fetch_wspr_candidates(cwslg_ctx *c, int ch_id, cwslg_wspr_candidate *dst, int max, int *n, uint64_t *start_epoch)
{
    static_assert(sizeof(cwslg_wspr_candidate) == sizeof(WsprCand), "candidate layout");
    return fetch_flat(c, ch_id, REC_CAND, CWSLG_LIST_WSPR, dst, sizeof(WsprCand), max, n, start_epoch);       // (sync_host.inc)
}

int cwslg_fetch_fst4w_candidates(cwslg_ctx *c, int ch_id, cwslg_fst4w_candidate *dst, int max, int *n, uint64_t *start_epoch)
{
    static_assert(sizeof(cwslg_fst4w_candidate) == sizeof(Fst4wCand), "candidate layout");
    return fetch_flat(c, ch_id, REC_CAND, CWSLG_LIST_FST4W, dst, sizeof(Fst4wCand), max, n, start_epoch);
}

int cwslg_long_sync_debug_fetch(cwslg_ctx *c, int ch_id, int what, void *dst, size_t cap_bytes, size_t *n_items)
{
    if (!c || !dst) return CWSLG_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    if (ch_id < 0 || ch_id >= (int)c->chans.size() || !c->chans[ch_id].open) return fail(c, CWSLG_ERR_ARG, "bad channel id");
    Channel &ch = c->chans[ch_id];
    if (!ch.have_frame || !ch.longbuf.d_block) return CWSLG_ERR_NO_FRAME;
    const LongWork &w = ch.longbuf.w;
    const void *src = nullptr;
    size_t items = 0;                                      // in floats
    if (ch.sync_wspr) {
        switch (what) {
        case 0: src = w.iq; items = 2 * (size_t)WSPR_M; break;                 // complex64[46080]
        case 1: src = w.ps; items = (size_t)WSPR_NFFTS * 512; break;            // [359][512], time-major
        case 2: src = w.vec; items = 411; break;                                // normalised smspec
        default: break;
        }
    } else if (ch.sync_fst4w) {
        switch (what) {
        case 3: src = w.vec; items = F4W_NNW; break;                            // normalised comb spectrum s2, indexed by i
        case 4: src = w.aux; items = 2 * (size_t)c->long_shared.f4w_nband; break;   // c_bigfft over the band, complex64
        default: break;
        }
    }
    if (!src) return fail(c, CWSLG_ERR_ARG, "bad selector");
    if (cap_bytes < items * 4) return fail(c, CWSLG_ERR_ARG, "destination too small");
    hipSetDevice(c->device);
    HIPCHK(c, hipMemcpyAsync(dst, src, items * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, sync_streams(c));
    if (n_items) *n_items = items;
    return CWSLG_OK;
}

} // extern "C"
