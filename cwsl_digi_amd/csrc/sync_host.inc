// sync_host.inc -- host glue of the FT8 sync stage (included by cwsl_gpu.hip inside the anonymous-namespace
// helpers' translation unit).  See sync_kernels.hpp for the algorithm and its "parity unpinned" status.
namespace {

int sync_ensure_shared(cwslg_ctx *c)
{
    if (c->sync_shared.d_tables) return CWSLG_OK;
    // twiddles ("spec v3", oracle/sync_oracle.c builds its own copy the same way): float(cos), float(-sin) of the
    // double angle; cardinal points exact (W^0 = (1,0), W128^32 = (0,-1)); the unpack table is stored as WH = 0.5 * W_2NZ (exact scaling);
    // W_15 / W_9 / W_5 / sin(2 pi / 3) are literals of the kernels (small_wr ..., sync_kernels.hpp), checked below against this host's libm
    constexpr double pi = 3.14159265358979323846;
    auto w = [&](int k, double n) { return make_float2((float)std::cos(2.0 * pi * k / n), (float)(-std::sin(2.0 * pi * k / n))); };
    auto half = [](float2 v) { return make_float2(0.5f * v.x, 0.5f * v.y); };
    // (BEFORE anything is allocated: a failed check must fail every later call too, not only the first)
    // the kernels carry W_9 (spec v2 stage 1, FT4), W_5 and sin(2 pi / 3) (spec v3 stage 1, FT8) as literals: this libm must produce the very same values
    auto same = [](float a, float b) { return std::memcmp(&a, &b, 4) == 0; };
    for (int k = 1; k <= 4; ++k)
        if (!same(w(k, 9.0).x, small_wr<9>(k)) || !same(w(k, 9.0).y, small_wi<9>(k)))
            return fail(c, CWSLG_ERR_HIP, "sync tables: W_9^%d computed on this host differs from the kernels' constants", k);
    for (int k = 1; k <= 2; ++k)
        if (!same(w(k, 5.0).x, w5_r(k)) || !same(w(k, 5.0).y, w5_i(k)))
            return fail(c, CWSLG_ERR_HIP, "sync tables: W_5^%d computed on this host differs from the kernels' constants", k);
    if (!same((float)(-std::sin(2.0 * pi / 3.0)), W3_S))
        return fail(c, CWSLG_ERR_HIP, "sync tables: sin(2 pi / 3) computed on this host differs from the kernels' constant");
    std::vector<float2> t;
    t.reserve(1920 + 64 + 1921 + 1152 + 1153);
    // FT8's W_1920 carries sync8's input scale: WN' = fl(fac * WN), fac = float(1/300) (the kernels then take the int16 samples as they are)
    const float fac = 1.0f / 300.0f;
    for (int k = 0; k < 1920; ++k) { const float2 v = (k == 0) ? make_float2(1.f, 0.f) : w(k, 1920.0); t.push_back(make_float2(fac * v.x, fac * v.y)); }
    for (int k = 0; k < 64; ++k) t.push_back(w(k, 128.0));
    for (int k = 0; k <= 1920; ++k) t.push_back(half(k == 0 ? make_float2(1.f, 0.f) : w(k, 3840.0)));
    t[1920] = make_float2(1.f, 0.f); t[1920 + 32] = make_float2(0.f, -1.f);
    const size_t ft8_count = t.size();
    for (int k = 0; k < 1152; ++k) t.push_back(w(k, 1152.0));
    for (int k = 0; k <= 1152; ++k) t.push_back(half(k == 0 ? make_float2(1.f, 0.f) : w(k, 2304.0)));
    t[ft8_count] = make_float2(1.f, 0.f);
    HIPCHK(c, hipMalloc(&c->sync_shared.d_tables, t.size() * sizeof(float2)));
    HIPCHK(c, hipMemcpy(c->sync_shared.d_tables, t.data(), t.size() * sizeof(float2), hipMemcpyHostToDevice));
    c->sync_shared.t.w1920 = c->sync_shared.d_tables;
    c->sync_shared.t.w128 = c->sync_shared.d_tables + 1920;
    c->sync_shared.t.w3840 = c->sync_shared.d_tables + 1920 + 64;
    c->sync_shared.t.win = nullptr;
    // FT4 set: W_1152 | W_2304 (k = 0..1152), Nuttall window (nuttal_window.f90 coefficients, double then float)
    float2 *t4 = c->sync_shared.d_tables + ft8_count;
    c->sync_shared.t4.w1920 = t4;
    c->sync_shared.t4.w128 = c->sync_shared.t.w128;
    c->sync_shared.t4.w3840 = t4 + 1152;
    std::vector<float> win(FT4_NFFT1);
    for (int i = 0; i < FT4_NFFT1; ++i)
        win[i] = (float)(0.3635819 - 0.4891775 * std::cos(2.0 * pi * i / 2304.0) + 0.1365995 * std::cos(4.0 * pi * i / 2304.0)
                         - 0.0106411 * std::cos(6.0 * pi * i / 2304.0));
    HIPCHK(c, hipMalloc(&c->sync_shared.d_win, win.size() * sizeof(float)));
    HIPCHK(c, hipMemcpy(c->sync_shared.d_win, win.data(), win.size() * sizeof(float), hipMemcpyHostToDevice));
    c->sync_shared.t4.win = c->sync_shared.d_win;
    return CWSLG_OK;
}

// Tables of the FT4 coherent sync stage, built exactly as oracle/ft4sync_oracle.c builds its own copy.
int ft4c_ensure_tables(cwslg_ctx *c)
{
    if (c->sync_shared.d_ft4c) return CWSLG_OK;
    const Ft4HostTables ht = ft4c_host_tables();
    const std::vector<float2> &t = ht.t;
    const std::vector<float> &win = ht.win;
    HIPCHK(c, hipMalloc(&c->sync_shared.d_ft4c, t.size() * sizeof(float2)));
    HIPCHK(c, hipMemcpy(c->sync_shared.d_ft4c, t.data(), t.size() * sizeof(float2), hipMemcpyHostToDevice));
    HIPCHK(c, hipMalloc(&c->sync_shared.d_ft4c_win, win.size() * sizeof(float)));
    HIPCHK(c, hipMemcpy(c->sync_shared.d_ft4c_win, win.data(), win.size() * sizeof(float), hipMemcpyHostToDevice));
    c->ft4_tables = ht.device(c->sync_shared.d_ft4c, c->sync_shared.d_ft4c_win);
    c->sync_shared.ft4_w32 = c->sync_shared.d_ft4c + ht.o32;
    return CWSLG_OK;
}

int ft4c_ensure_channel(cwslg_ctx *c, Channel &ch)
{
    SyncChannelBuffers &b = ch.syncbuf;
    if (b.d_ft4c) return CWSLG_OK;
    const size_t y = (size_t)F4C_N2 * sizeof(float2), cx = ((size_t)(F4C_N2 + 1) * sizeof(float2) + 255) & ~size_t(255);
    const size_t cd = (size_t)F4C_NP * sizeof(float2);
    const size_t rec = ((size_t)b.max_cand * 3 * sizeof(Ft4Rec) + 255) & ~size_t(255);
    const size_t nrec = ((size_t)b.max_cand * sizeof(int) + 255) & ~size_t(255);
    HIPCHK(c, hipMalloc((void **)&b.d_ft4c, y + cx + cd + rec + nrec));
    char *p = b.d_ft4c;
    b.d_y = (float2 *)p; p += y;
    b.d_cx = (float2 *)p; p += cx;
    b.d_cd_dbg = (float2 *)p; p += cd;
    b.d_rec = p; p += rec;
    b.d_nrec = (int *)p;
    return CWSLG_OK;
}

// A record array of the FT4 chain -- soft-bit (ft4soft_kernels.hpp), decode (ldpc_kernels.hpp) or OSD records (osd_kernels.hpp's third addressing
// mode), [max_cand][3] in d_rec's slot layout, an allocation of its own: it exists only while its stage is queued (a boundary without it frees
// it), goes with the channel (sync_free_channel) and follows max_cand (sync_ensure_channel frees everything when it changes).  A change either
// way clears the kind's stamp: nothing to fetch until the stage has run on the new array.
int ensure_record_array(cwslg_ctx *c, void **arr, uint64_t &stamp, size_t bytes, bool want)
{
    if ((*arr != nullptr) == want) return CWSLG_OK;
    stamp = 0;
    if (!want) { (void)hipFree(*arr); *arr = nullptr; return CWSLG_OK; }
    HIPCHK(c, hipMalloc(arr, bytes));
    return CWSLG_OK;
}

int sync_ensure_channel(cwslg_ctx *c, Channel &ch)
{
    SyncChannelBuffers &b = ch.syncbuf;
    const SyncConfig &cfg = c->sync_cfg;
    const int want_bins = ch.sync_ft4 ? FT4_ROW : cfg.nbins;
    const bool want_soft = cfg.kept.ft8_soft && ch.sync_ft8;      // the soft-bit records exist only while the feature is on (a later enable reallocates)
    const bool want_msg = want_soft && cfg.kept.ft8_decode;       // ... and so do the decode records
    const bool want_osd = want_msg && cfg.kept.ft8_osd;           // ... and the OSD records
    if (b.d_block && b.nbins == want_bins && b.max_cand == cfg.max_cand && b.ft4 == ch.sync_ft4 && (b.d_soft != nullptr) == want_soft &&
        (b.d_msg != nullptr) == want_msg && (b.d_osd != nullptr) == want_osd)
        return CWSLG_OK;
    sync_free_channel(b);
    for (int k = REC_CAND + 1; k < REC_KINDS; ++k) ch.stamp[k] = 0;      // (every stamp but the list's)
    const size_t sp = ((size_t)(ch.sync_ft4 ? FT4_NHSYM : FT8_NHSYM) * want_bins * sizeof(float) + 255) & ~size_t(255);
    const size_t vec = ((size_t)(FT8_NH1 + 1) * 4 + 255) & ~size_t(255);
    const size_t cand = ((size_t)cfg.max_cand * sizeof(SyncChannelBuffers::Cand) + 255) & ~size_t(255);
    const size_t soft = want_soft ? (size_t)cfg.max_cand * sizeof(Ft8SoftRec) : 0;
    const size_t msg = want_msg ? (size_t)cfg.max_cand * sizeof(Ft8MsgRec) : 0;
    const size_t msg_pad = want_osd ? (msg + 7) & ~size_t(7) : msg;      // (the OSD records hold a float: keep them 8-byte aligned)
    const size_t osd = want_osd ? (size_t)cfg.max_cand * sizeof(OsdRec) : 0;
    HIPCHK(c, hipMalloc((void **)&b.d_block, sp + 4 * vec + cand + 256 + soft + msg_pad + osd));
    char *p = b.d_block;
    b.d_spectra = (float *)p; p += sp;
    b.d_red = (float *)p; p += vec;
    b.d_red2 = (float *)p; p += vec;
    b.d_jpeak = (int *)p; p += vec;
    b.d_jpeak2 = (int *)p; p += vec;
    b.d_cand = (SyncChannelBuffers::Cand *)p; p += cand;
    b.d_ncand = (int *)p; p += 256;
    if (want_soft) { b.d_soft = (Ft8SoftRec *)p; p += soft; }
    if (want_msg) { b.d_msg = (Ft8MsgRec *)p; p += msg_pad; }
    if (want_osd) b.d_osd = (OsdRec *)p;
    b.nbins = want_bins;
    b.max_cand = cfg.max_cand;
    b.ft4 = ch.sync_ft4;
    HIPCHK(c, hipMemsetAsync(b.d_ncand, 0, 256, c->stream));
    return CWSLG_OK;
}

// ldpc_decode_kernel's three addressing modes, one launcher each: what a mode does not use is null / 0 here and nowhere else.
//   FT8 chain: one wave per candidate of n_chan channels, records behind the soft-bit records
void ldpc_launch_ft8(hipStream_t st, const void *tables, const SyncWork *works, Ft8SoftRec *const *soft, Ft8MsgRec *const *msg, size_t n_chan, int max_cand,
                     int max_iter, int min_nsync)
{
    hipLaunchKernelGGL(ldpc_decode_kernel, dim3((unsigned)((max_cand + LDPC_WAVES - 1) / LDPC_WAVES), (unsigned)n_chan), dim3(64 * LDPC_WAVES), 0, st, works, soft, msg,
                       (const float *)nullptr, (Ft8MsgRec *)nullptr, 0, max_cand, max_iter, min_nsync, (const LdpcTables *)tables, (const Ft4Work *)nullptr,
                       (Ft4SoftRec *const *)nullptr, (Ft4MsgRec *const *)nullptr, 0);
}
//   flat: n sets of 174 metrics, no gate
void ldpc_launch_flat(hipStream_t st, const void *tables, const float *llr, Ft8MsgRec *out, int n, int max_iter)
{
    hipLaunchKernelGGL(ldpc_decode_kernel, dim3((unsigned)((n + LDPC_WAVES - 1) / LDPC_WAVES), 1), dim3(64 * LDPC_WAVES), 0, st, (const SyncWork *)nullptr,
                       (Ft8SoftRec *const *)nullptr, (Ft8MsgRec *const *)nullptr, llr, out, n, 0, max_iter, 0, (const LdpcTables *)tables, (const Ft4Work *)nullptr,
                       (Ft4SoftRec *const *)nullptr, (Ft4MsgRec *const *)nullptr, 0);
}
//   FT4 chain: one wave per (record slot, metric set) of n_chan channels, 9 max_cand waves per channel
void ldpc_launch_ft4(hipStream_t st, const void *tables, const Ft4Work *works4, Ft4SoftRec *const *soft4, Ft4MsgRec *const *msg4, size_t n_chan, int max_cand,
                     int max_iter, int min_nsync, int min_nqual)
{
    hipLaunchKernelGGL(ldpc_decode_kernel, dim3((unsigned)((9 * max_cand + LDPC_WAVES - 1) / LDPC_WAVES), (unsigned)n_chan), dim3(64 * LDPC_WAVES), 0, st,
                       (const SyncWork *)nullptr, (Ft8SoftRec *const *)nullptr, (Ft8MsgRec *const *)nullptr, (const float *)nullptr, (Ft8MsgRec *)nullptr, 0, max_cand,
                       max_iter, min_nsync, (const LdpcTables *)tables, works4, soft4, msg4, min_nqual);
}

// osd_decode_kernel's three addressing modes
//   FT8 chain: one wave per candidate of n_chan channels, behind the decode records it gates on
void osd_launch_ft8(hipStream_t st, const void *gen, const SyncWork *works, Ft8SoftRec *const *soft, Ft8MsgRec *const *msg, OsdRec *const *osd, size_t n_chan,
                    int max_cand, int order, int min_nsync)
{
    hipLaunchKernelGGL(osd_decode_kernel, dim3((unsigned)((max_cand + OSD_WAVES - 1) / OSD_WAVES), (unsigned)n_chan), dim3(64 * OSD_WAVES), 0, st, works, soft, msg, osd,
                       (const float *)nullptr, (OsdRec *)nullptr, 0, max_cand, order, min_nsync, (const OsdGen *)gen, (const Ft4Work *)nullptr,
                       (Ft4SoftRec *const *)nullptr, (Ft4MsgRec *const *)nullptr, (Ft4OsdRec *const *)nullptr, 0);
}
//   flat: n sets of 174 metrics, no gate
void osd_launch_flat(hipStream_t st, const void *gen, const float *llr, OsdRec *out, int n, int order)
{
    hipLaunchKernelGGL(osd_decode_kernel, dim3((unsigned)((n + OSD_WAVES - 1) / OSD_WAVES), 1), dim3(64 * OSD_WAVES), 0, st, (const SyncWork *)nullptr,
                       (Ft8SoftRec *const *)nullptr, (Ft8MsgRec *const *)nullptr, (OsdRec *const *)nullptr, llr, out, n, 0, order, 0, (const OsdGen *)gen,
                       (const Ft4Work *)nullptr, (Ft4SoftRec *const *)nullptr, (Ft4MsgRec *const *)nullptr, (Ft4OsdRec *const *)nullptr, 0);
}
//   FT4 chain: one wave per (record slot, metric set) of n_chan channels, 9 max_cand waves per channel, behind the decode records it gates on
void osd_launch_ft4(hipStream_t st, const void *gen, const Ft4Work *works4, Ft4SoftRec *const *soft4, Ft4MsgRec *const *msg4, Ft4OsdRec *const *osd4, size_t n_chan,
                    int max_cand, int order, int min_nsync, int min_nqual)
{
    hipLaunchKernelGGL(osd_decode_kernel, dim3((unsigned)((9 * max_cand + OSD_WAVES - 1) / OSD_WAVES), (unsigned)n_chan), dim3(64 * OSD_WAVES), 0, st,
                       (const SyncWork *)nullptr, (Ft8SoftRec *const *)nullptr, (Ft8MsgRec *const *)nullptr, (OsdRec *const *)nullptr, (const float *)nullptr,
                       (OsdRec *)nullptr, 0, max_cand, order, min_nsync, (const OsdGen *)gen, works4, soft4, msg4, osd4, min_nqual);
}

// The record arrays of one chain (soft-bit, decode, OSD records) of the channels queued at a boundary, one pointer per channel and stage that is on,
// in the order of the chain's descriptors.  place() writes the three pointer tables behind the descriptors of the chain's work buffer -- soft,
// then decode, then OSD; a stage that is off adds no byte -- and keeps the device addresses the kernels take.
template <class Soft, class Msg, class Osd> struct ChainArrays {
    std::vector<Soft *> soft;
    std::vector<Msg *> msg;
    std::vector<Osd *> osd;
    Soft *const *d_soft = nullptr;
    Msg *const *d_msg = nullptr;
    Osd *const *d_osd = nullptr;
    size_t bytes() const { return (soft.size() + msg.size() + osd.size()) * sizeof(void *); }
    void place(const WorkBuf *wb, size_t desc_bytes)
    {
        void **h = (void **)((char *)wb->h + desc_bytes), **d = (void **)((char *)wb->d + desc_bytes);
        if (!soft.empty()) std::memcpy(h, soft.data(), soft.size() * sizeof(void *));
        if (!msg.empty()) std::memcpy(h + soft.size(), msg.data(), msg.size() * sizeof(void *));
        if (!osd.empty()) std::memcpy(h + soft.size() + msg.size(), osd.data(), osd.size() * sizeof(void *));
        d_soft = (Soft *const *)d;
        d_msg = (Msg *const *)(d + soft.size());
        d_osd = (Osd *const *)(d + soft.size() + msg.size());
    }
};

// Run the sync stage on the frames finalised by this boundary: FT8 channels through the Costas search, FT4
// channels through getcandidates4's spectral-peak search.  Other modes have no sync stage.
int sync_launch(cwslg_ctx *c, const std::vector<int> &emitted)
{
    int rc = sync_ensure_shared(c);
    if (rc) return rc;
    const SyncConfig &cfg = c->sync_cfg;
    std::vector<SyncWork> works8, works4;
    std::vector<Ft4Work> works4c;
    ChainArrays<Ft8SoftRec, Ft8MsgRec, OsdRec> a8;            // the FT8 chain's record arrays, one per FT8 channel and stage that is on, in works8's order
    ChainArrays<Ft4SoftRec, Ft4MsgRec, Ft4OsdRec> a4;         // the FT4 chain's (behind the coherent stage), in works4c's order
    // the stages' switches by record kind: records_queued (record_kinds.hpp) says which of them run for a channel, each behind the one it reads from
    const bool on[REC_KINDS] = {true, cfg.kept.ft4_coherent, cfg.kept.ft8_soft, cfg.kept.ft8_decode, cfg.kept.ft8_osd, cfg.kept.ft4_soft, cfg.kept.ft4_decode,
                                cfg.kept.ft4_osd};
    for (int id : emitted) {
        Channel &ch = c->chans[id];
        if (!ch.sync_ft8 && !ch.sync_ft4) continue;
        rc = sync_ensure_channel(c, ch);
        if (rc) return rc;
        SyncWork w{};
        w.frame = ch.d_i16;
        w.spectra = ch.syncbuf.d_spectra;
        w.red = ch.syncbuf.d_red; w.red2 = ch.syncbuf.d_red2;
        w.jpeak = ch.syncbuf.d_jpeak; w.jpeak2 = ch.syncbuf.d_jpeak2;
        w.cand = ch.syncbuf.d_cand; w.ncand = ch.syncbuf.d_ncand;
        if (ch.fin_fused) { w.fin = ch.fused_fin; ch.fin_fused = false; }       // the spectra kernel finalises this frame first (boundary_locked)
        (ch.sync_ft8 ? works8 : works4).push_back(w);
        const unsigned queued = records_queued(ch.sync_ft8, ch.sync_ft4, on);
        auto runs = [&](int k) { return (queued & rec_bit(k)) != 0; };
        SyncChannelBuffers &b = ch.syncbuf;
        if (runs(REC_FT4SYNC)) {
            if ((rc = ft4c_ensure_tables(c)) != CWSLG_OK || (rc = ft4c_ensure_channel(c, ch)) != CWSLG_OK) return rc;
            Ft4Work f{};
            f.frame = ch.d_i16; f.y = b.d_y; f.cx = b.d_cx;
            f.cand = b.d_cand; f.ncand = b.d_ncand;
            f.rec = (Ft4Rec *)b.d_rec; f.nrec = b.d_nrec; f.cd_dbg = b.d_cd_dbg;
            works4c.push_back(f);
        }
        if (ch.sync_ft4) {
            const size_t slots = (size_t)b.max_cand * 3;
            if ((rc = ensure_record_array(c, (void **)&b.d_ft4soft, ch.stamp[REC_SOFT4], slots * sizeof(Ft4SoftRec), runs(REC_SOFT4))) != CWSLG_OK) return rc;
            if ((rc = ensure_record_array(c, (void **)&b.d_ft4msg, ch.stamp[REC_MSG4], slots * sizeof(Ft4MsgRec), runs(REC_MSG4))) != CWSLG_OK) return rc;
            if ((rc = ensure_record_array(c, (void **)&b.d_ft4osd, ch.stamp[REC_OSD4], slots * sizeof(Ft4OsdRec), runs(REC_OSD4))) != CWSLG_OK) return rc;
        }
        // what is queued now belongs to this frame; a stage that is off keeps its OLD stamp: nothing of it to fetch (record_kinds.hpp)
        for (int k = 0; k < REC_KINDS; ++k)
            if (runs(k)) ch.stamp[k] = ch.frame_t0;
        if (runs(REC_SOFT8)) a8.soft.push_back(b.d_soft);
        if (runs(REC_MSG8)) a8.msg.push_back(b.d_msg);
        if (runs(REC_OSD8)) a8.osd.push_back(b.d_osd);
        if (runs(REC_SOFT4)) a4.soft.push_back(b.d_ft4soft);
        if (runs(REC_MSG4)) a4.msg.push_back(b.d_ft4msg);
        if (runs(REC_OSD4)) a4.osd.push_back(b.d_ft4osd);
    }
    if (works8.empty() && works4.empty()) return CWSLG_OK;
    const size_t n8 = works8.size(), n4 = works4.size();
    // the FT8 chain's record pointers ride behind the descriptors in the same buffer (nothing is added while the feature is off)
    const size_t wb_bytes = (n8 + n4) * sizeof(SyncWork) + a8.bytes();
    WorkBuf *wb = acquire_workbuf(c, wb_bytes);
    if (!wb) return fail(c, CWSLG_ERR_NOMEM, "work buffer allocation failed");
    if (n8) std::memcpy(wb->h, works8.data(), n8 * sizeof(SyncWork));
    if (n4) std::memcpy((SyncWork *)wb->h + n8, works4.data(), n4 * sizeof(SyncWork));
    a8.place(wb, (n8 + n4) * sizeof(SyncWork));
    HIPCHK(c, upload_workbuf(c, wb, wb_bytes));
    // one wave per candidate behind whichever search form wrote d_cand / d_ncand (the count is read on the device); its time is part of the
    // stage's span (stats.sync_ms), not of the search's own
    auto launch_soft = [&](hipStream_t st) {
        if (a8.soft.empty()) return;
        hipLaunchKernelGGL(ft8_softbits_kernel, dim3((unsigned)((cfg.max_cand + FT8S_WAVES - 1) / FT8S_WAVES), (unsigned)n8), dim3(64 * FT8S_WAVES), 0, st,
                           (const SyncWork *)wb->d, a8.d_soft, cfg.nbins, cfg.max_cand);
        // the decode: one wave per candidate behind the metrics it reads (same grid, same device-side count); counted as a launch of its own
        if (a8.msg.empty()) return;
        ldpc_launch_ft8(st, c->sync_shared.d_ldpc, (const SyncWork *)wb->d, a8.d_soft, a8.d_msg, n8, cfg.max_cand, cfg.kept.ldpc_max_iter, cfg.kept.ldpc_min_nsync);
        c->stats.sync_launches++;
        // OSD: one wave per candidate behind the decode records it gates on; counted as a launch of its own
        if (a8.osd.empty()) return;
        osd_launch_ft8(st, c->sync_shared.d_osdgen, (const SyncWork *)wb->d, a8.d_soft, a8.d_msg, a8.d_osd, n8, cfg.max_cand, cfg.kept.osd_order, cfg.kept.osd_min_nsync);
        c->stats.sync_launches++;
    };
    WorkBuf *wb4 = nullptr;
    if (!works4c.empty()) {
        // (the FT4 chain's record pointers ride behind the descriptors, as the FT8 ones do above)
        const size_t wb4_bytes = works4c.size() * sizeof(Ft4Work) + a4.bytes();
        wb4 = acquire_workbuf(c, wb4_bytes);
        if (!wb4) return fail(c, CWSLG_ERR_NOMEM, "work buffer allocation failed");
        std::memcpy(wb4->h, works4c.data(), works4c.size() * sizeof(Ft4Work));
        a4.place(wb4, works4c.size() * sizeof(Ft4Work));
        HIPCHK(c, upload_workbuf(c, wb4, wb4_bytes));
    }
    hipEvent_t ea, eb;
    // CWSLG_SYNC_VARIANT bit 3: the candidate kernel on a side stream, overlapping the next demod launch.  Measured and left off:
    // 4.47-4.56 against 4.10-4.12 ms per step at 512 slots, no change at 4096 (the overlapped demod kernel slows by more than the
    // 0.1 ms the candidate kernel takes).
    // CWSLG_SYNC_VARIANT bit 5: the WHOLE FT8 chain (spectra, Costas search, candidates) on the side stream, so that it runs next to
    // the demodulation of the following slot (boundary_locked makes the next finalise wait for it: the int16 frames are its input).
    // Measured and left off: the two do overlap (demod 21.2 -> 24.2 ms, sync 8.9 -> 19.8 ms per launch at 4096 slots) and the step
    // takes 31.6-31.8 against 31.3-31.5 ms (4.25 against 4.05 at 512): the chip has no idle capacity for the second stream to use.
    const bool chain_async = n8 && !n4 && (c->sync_variant & 32);
    const bool cand_async = n8 && (c->sync_variant & 8) && !chain_async;
    if (n8 && c->cand_pending) {                                // the previous boundary's candidate kernel still reads red / jpeak
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->cand_done, 0));
        c->cand_pending = false;
    }
    hipStream_t s8 = c->stream;
    if (chain_async) {
        s8 = c->side;
        HIPCHK(c, hipEventRecord(c->sync2d_done, c->stream));   // behind the finalise kernel and the descriptor copy
        HIPCHK(c, hipStreamWaitEvent(c->side, c->sync2d_done, 0));
        span_begin_on(c, 2, c->side, &ea, &eb);
    } else {
        span_begin(c, 2, &ea, &eb);
    }
    if (n8) {
        const SyncWork *d8 = (const SyncWork *)wb->d;
        const unsigned nbands = (unsigned)((cfg.ib - cfg.ia + 1 + SYNC_BAND - 1) / SYNC_BAND);
#if CWSLG_LAB
        if (c->sync_variant & 2)           // CWSLG_SYNC_VARIANT bit 1: the round-1 spectra kernel (same bits)
            hipLaunchKernelGGL((symbol_spectra_kernel<15, FT8_NSPS, FT8_NSTEP, false>), dim3(FT8_NHSYM, (unsigned)n8), dim3(256), 0,
                               s8, d8, c->sync_shared.t, cfg.nbins);
        else
#endif
        {
        hipEvent_t pa = nullptr, pb = nullptr;                 // the two kernels of the FT8 chain are also timed apart (bench.py: each against its own bound)
        if (s8 == c->stream) span_begin(c, 3, &pa, &pb);
        const int jper8 = spectra_jper(FT8_NHSYM, n8);
        // every FT8 channel of a boundary is finalised by the spectra kernel or none is (boundary_locked decides by context-wide conditions)
        bool fused8 = works8[0].fin.frame != nullptr;
        for (const SyncWork &sw : works8) if ((sw.fin.frame != nullptr) != fused8) return fail(c, CWSLG_ERR_ARG, "mixed fused / separate finalise in one launch");
        const dim3 g8((FT8_NHSYM + jper8 - 1) / jper8, (unsigned)n8);
        if (!fused8) {
            // (product library: every FT8 frame that reaches the sync stage is finalised by the spectra kernel; the form that reads a finished int16 frame
            // exists in the lab library and in A/B builds with -DCWSLG_FUSE_FIN_DEFAULT=0)
#if CWSLG_LAB || !CWSLG_FUSE_FIN_DEFAULT
            hipLaunchKernelGGL((symbol_spectra_v2_kernel<15, FT8_NSPS, FT8_NSTEP, false, 0>), g8, dim3(256), 0, s8, d8, c->sync_shared.t, cfg.nbins, FT8_NHSYM, jper8);
#else
            return fail(c, CWSLG_ERR_ARG, "FT8 frame reached the sync stage without its finalise");
#endif
        }
#if CWSLG_LAB || CWSLG_FUSE_MODE_DEFAULT == 2
        else if (c->fuse_mode == 2)        // CWSLG_FUSE_MODE=2 (lab library): the windows from an LDS ring -- measured alternative, 5.2 against 4.5 ms
            hipLaunchKernelGGL((symbol_spectra_v2_kernel<15, FT8_NSPS, FT8_NSTEP, false, 2>), g8, dim3(256), 0, s8, d8, c->sync_shared.t, cfg.nbins, FT8_NHSYM, jper8);
#endif
        else
            hipLaunchKernelGGL((symbol_spectra_v2_kernel<15, FT8_NSPS, FT8_NSTEP, false, 1>), g8, dim3(256), 0, s8, d8, c->sync_shared.t, cfg.nbins, FT8_NHSYM, jper8);
        span_end(c, pb);
        }
        // Two forms of the same search + selection (same sums, same order: same bits), chosen by how many channels this boundary carries:
        // one workgroup per channel walking all bands (sliding LDS window, prefetch, fused selection) once there are enough channels to
        // fill the chip's workgroup slots (two per CU); below that, one workgroup per band and the selection as a second launch.
        const bool per_channel = n8 >= (size_t)2 * (size_t)c->cu_count;
#if CWSLG_LAB
        if (!(c->sync_variant & (1 | 64 | 128))) {
#endif
        hipEvent_t qa = nullptr, qb = nullptr;
        if (s8 == c->stream) span_begin(c, 4, &qa, &qb);
        if (per_channel) {
            hipLaunchKernelGGL(ft8_sync_chan_kernel, dim3((unsigned)n8), dim3(SYNCC_NT), 0, s8, d8, cfg.ia, cfg.ib, cfg.nbins, cfg.syncmin, cfg.max_cand, cfg.kept.order);
        } else {
            hipLaunchKernelGGL(ft8_sync2d_v3_kernel, dim3(nbands, (unsigned)n8), dim3(SYNC2D_NT), 0, s8, d8, cfg.ia, cfg.ib, cfg.nbins);
            hipLaunchKernelGGL(ft8_candidates_kernel<1024>, dim3((unsigned)n8), dim3(1024), 0, s8, d8, cfg.ia, cfg.ib, cfg.syncmin, cfg.max_cand, cfg.kept.order);
        }
        span_end(c, qb);
        launch_soft(s8);
#if CWSLG_LAB
        } else {
        // the three-launch forms (one workgroup per 32-bin band, then one per channel for the selection), all with the same bits:
        // bit 0 round 1's search, bit 6 round 2's (hipcc-scheduled LDS reads), bit 7 the hand-scheduled search as its own launch.
        // Measured at 4096 slots, same box: sync stage 9.19 (bit 6), 8.89-8.91 (bit 7), 8.67 ms (the fused kernel above).
        if (c->sync_variant & 1)
            hipLaunchKernelGGL(ft8_sync2d_kernel, dim3(nbands, (unsigned)n8), dim3(SYNC2D_NT), 0, s8, d8, cfg.ia, cfg.ib, cfg.nbins);
        else if (c->sync_variant & 64)
            hipLaunchKernelGGL(ft8_sync2d_v2_kernel, dim3(nbands, (unsigned)n8), dim3(SYNC2D_NT), 0, s8, d8, cfg.ia, cfg.ib, cfg.nbins);
        else
            hipLaunchKernelGGL(ft8_sync2d_v3_kernel, dim3(nbands, (unsigned)n8), dim3(SYNC2D_NT), 0, s8, d8, cfg.ia, cfg.ib, cfg.nbins);
        hipStream_t cs = s8;
        hipEvent_t sa = nullptr, sb = nullptr;
        if (cand_async) {
            cs = c->side;
            HIPCHK(c, hipEventRecord(c->sync2d_done, c->stream));
            HIPCHK(c, hipStreamWaitEvent(c->side, c->sync2d_done, 0));
            span_begin_on(c, 2, c->side, &sa, &sb);
        }
        if (c->sync_variant & 4)           // CWSLG_SYNC_VARIANT bit 2: 256 threads per channel, as in round 1
            hipLaunchKernelGGL(ft8_candidates_kernel<256>, dim3((unsigned)n8), dim3(256), 0, cs, d8, cfg.ia, cfg.ib,
                               cfg.syncmin, cfg.max_cand, cfg.kept.order);
        else
            hipLaunchKernelGGL(ft8_candidates_kernel<1024>, dim3((unsigned)n8), dim3(1024), 0, cs, d8, cfg.ia, cfg.ib,
                               cfg.syncmin, cfg.max_cand, cfg.kept.order);
        launch_soft(cs);
        if (cand_async) {
            if (sb) hipEventRecord(sb, c->side);
            HIPCHK(c, hipEventRecord(c->cand_done, c->side));
            c->cand_pending = true;
        }
        }
#endif
    }
    if (n4) {
        const SyncWork *d4 = (const SyncWork *)wb->d + n8;
        // getcandidates4: nfa = int(fa/df) clamped to nint(200/df); nfb = int(fb/df) clamped to nint(4910/df)
        const float df4 = 12000.0f / (float)FT4_NFFT1;
        int nfa = (int)((float)cfg.f_lo_hz / df4), nfb = (int)((float)cfg.f_hi_hz / df4);
        nfa = std::max(nfa, (int)std::lround(200.0f / df4));
        nfb = std::min(nfb, (int)std::lround(4910.0f / df4));
        const int jper4 = spectra_jper(FT4_NHSYM, n4);
#if CWSLG_LAB
        if (c->sync_variant & 2)
            hipLaunchKernelGGL((symbol_spectra_kernel<9, FT4_NFFT1, FT4_NSTEP, true>), dim3(FT4_NHSYM, (unsigned)n4), dim3(256), 0,
                               c->stream, d4, c->sync_shared.t4, FT4_ROW);
        else
#endif
        hipLaunchKernelGGL((symbol_spectra_v2_kernel<9, FT4_NFFT1, FT4_NSTEP, true>), dim3((FT4_NHSYM + jper4 - 1) / jper4, (unsigned)n4), dim3(256), 0,
                           c->stream, d4, c->sync_shared.t4, FT4_ROW, FT4_NHSYM, jper4);
        hipLaunchKernelGGL(ft4_candidates_kernel, dim3((unsigned)n4), dim3(256), 0, c->stream, d4, nfa, nfb,
                           c->sync_cfg.syncmin_ft4, cfg.max_cand, cfg.kept.order);
        if (c->sync_cfg.kept.ft4_coherent) {
            // the coherent stage of ft4_decode on every candidate: frame spectrum, then one workgroup per candidate
            const Ft4Work *f4 = (const Ft4Work *)wb4->d;
#if CWSLG_LAB
            if (c->ft4_dft_valu)          // CWSLG_FT4_DFT=valu: the VALU form of the same chains (measured alternative)
                hipLaunchKernelGGL(ft4_dft567_kernel, dim3((F4C_NA + 4 * F4C_CPT - 1) / (4 * F4C_CPT), (unsigned)n4), dim3(256), 0, c->stream, f4, c->ft4_tables);
            else
#endif
            hipLaunchKernelGGL(ft4_dft567_mfma_kernel, dim3(9, (unsigned)n4), dim3(256), 0, c->stream, f4, c->ft4_tables);
            hipLaunchKernelGGL(ft4_fft64_unpack_kernel, dim3(284, (unsigned)n4), dim3(64), 0, c->stream, f4, c->ft4_tables);
            hipLaunchKernelGGL(ft4_refine_kernel, dim3((unsigned)cfg.max_cand, (unsigned)n4), dim3(256), 0, c->stream, f4, c->ft4_tables, cfg.max_cand);
            // soft bits: one workgroup per record slot behind the refinement; nrec and the candidate count are read on the device
            if (!a4.soft.empty())
                ft4_softbits_launch(c->stream, f4, a4.d_soft, c->ft4_tables, c->sync_shared.ft4_w32, cfg.max_cand, (int)n4);
            // the decode: one wave per (record slot, metric set) behind the metrics it reads, the counts read on the device as the launch above
            // reads them; counted as a launch of its own, as the FT8 decode's is
            if (!a4.msg.empty()) {
                ldpc_launch_ft4(c->stream, c->sync_shared.d_ldpc, f4, a4.d_soft, a4.d_msg, n4, cfg.max_cand, cfg.kept.ldpc4_max_iter, cfg.kept.ldpc4_min_nsync,
                                cfg.kept.ldpc4_min_nqual);
                c->stats.sync_launches++;
                // OSD: one wave per (record slot, metric set) behind the decode records it gates on; counted as a launch of its own
                if (!a4.osd.empty()) {
                    osd_launch_ft4(c->stream, c->sync_shared.d_osdgen, f4, a4.d_soft, a4.d_msg, a4.d_osd, n4, cfg.max_cand, cfg.kept.osd4_order, cfg.kept.osd4_min_nsync,
                                   cfg.kept.osd4_min_nqual);
                    c->stats.sync_launches++;
                }
            }
        }
    }
    if (chain_async) {
        if (eb) hipEventRecord(eb, c->side);
        HIPCHK(c, hipEventRecord(c->cand_done, c->side));
        c->cand_pending = true;
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(wb->done, c->side));
        wb->in_flight = true;
        c->stats.sync_launches++;
        return CWSLG_OK;
    }
    span_end(c, eb);
    HIPCHK(c, hipGetLastError());
    if (cand_async) {
        // the descriptor buffer is read on both streams: its "done" event goes behind the last reader of either
        HIPCHK(c, hipEventRecord(c->sync_tail, c->stream));
        HIPCHK(c, hipStreamWaitEvent(c->side, c->sync_tail, 0));
        HIPCHK(c, hipEventRecord(wb->done, c->side));
    } else {
        HIPCHK(c, hipEventRecord(wb->done, c->stream));
    }
    wb->in_flight = true;
    if (wb4) { HIPCHK(c, hipEventRecord(wb4->done, c->stream)); wb4->in_flight = true; }
    c->stats.sync_launches++;
    return CWSLG_OK;
}

// ---- the list and record fetches ------------------------------------------------------------------------------------------------------------
// Lists and records are handed out the way cwslg_fetch_frame hands a frame out (ABI 5): under the context mutex only the pointers are read and
// a ticket of the channel's group is taken (fetch_begin); the copies run on a fetch stream behind the group's generation event with the mutex
// released (a fetch during a 30 ms demod launch does not block every pusher), and the group's next boundary -- the next writer of the buffers --
// waits for the ticket.  *start_epoch is the start epoch of the frame the records were computed from.  WHAT may be handed out, and under which
// epoch, is the kind table's business (record_kinds.hpp); HOW it is copied out is one of two bodies: fetch_flat (a count, then that many
// items) and fetch_walk (the FT4 chain's slot layout, compacted by the nrec walk).

// The array of kind k (REC_CAND: the list, inside d_block; REC_FT4SYNC: d_rec, inside d_ft4c)
const void *record_array(const SyncChannelBuffers &b, int k)
{
    switch (k) {
    case REC_CAND: return b.d_cand;
    case REC_FT4SYNC: return b.d_rec;
    case REC_SOFT8: return b.d_soft;
    case REC_MSG8: return b.d_msg;
    case REC_OSD8: return b.d_osd;
    case REC_SOFT4: return b.d_ft4soft;
    case REC_MSG4: return b.d_ft4msg;
    case REC_OSD4: return b.d_ft4osd;
    }
    return nullptr;
}

// records_epoch on a channel.  list_block: the block that holds the list in question -- syncbuf.d_block, or longbuf.d_block for a 120 s list.
uint64_t channel_records_epoch(const Channel &ch, int k, const void *list_block, bool with_frame = false)
{
    unsigned present = list_block ? rec_bit(REC_CAND) : 0;
    for (int j = REC_CAND + 1; j < REC_KINDS; ++j)
        if (record_array(ch.syncbuf, j)) present |= rec_bit(j);
    return records_epoch(k, ch.have_frame, ch.frame_t0, ch.stamp, present, with_frame);
}

struct RecSource {
    const void *rec = nullptr;          // the records (flat: [cap]; walk: [cap][3])
    const int *cnt = nullptr;           // the list's count
    const int *nrec = nullptr;          // walk: records per candidate, [cap]
    int cap = 0;                        // the list limit the arrays were sized for
};

// The part of a fetch under the context mutex: channel, mode gate, the rule, *start_epoch, the device pointers and the ticket.  long_list: 0, or
// CWSLG_LIST_WSPR / CWSLG_LIST_FST4W for the list of a 120 s channel (kind REC_CAND, buffers of the channel's longbuf).
int fetch_begin(cwslg_ctx *c, int ch_id, int k, int long_list, uint64_t *start_epoch, RecSource &s, ResultFetch &rf)
{
    std::lock_guard<std::mutex> g(c->mu);
    if (ch_id < 0 || ch_id >= (int)c->chans.size() || !c->chans[ch_id].open) return fail(c, CWSLG_ERR_ARG, "bad channel id");
    Channel &ch = c->chans[ch_id];
    const RecKindRow &row = kRecKinds[k];
    if (long_list) {
        if (long_list == CWSLG_LIST_WSPR ? !ch.sync_wspr : !ch.sync_fst4w)
            return fail(c, CWSLG_ERR_MODE, "channel mode %s has no such candidate list", ch.mode.c_str());
    } else if (row.gate && !(row.chain == CHAIN_FT8 ? ch.sync_ft8 : ch.sync_ft4)) {
        return fail(c, CWSLG_ERR_MODE, row.gate, ch.mode.c_str());
    }
    const uint64_t t0 = channel_records_epoch(ch, k, long_list ? ch.longbuf.d_block : ch.syncbuf.d_block);
    if (!t0) return CWSLG_ERR_NO_FRAME;
    hipSetDevice(c->device);
    if (start_epoch) *start_epoch = t0;
    if (long_list) s = RecSource{ch.longbuf.w.cand, ch.longbuf.w.ncand, nullptr, long_list == CWSLG_LIST_WSPR ? (int)WSPR_MAXCAND : (int)F4W_MAXCAND};
    else s = RecSource{record_array(ch.syncbuf, k), ch.syncbuf.d_ncand, ch.syncbuf.d_nrec, ch.syncbuf.max_cand};
    return begin_result_fetch(c, ch, rf);
}

// Flat body: the count and min(max, cap) items in one synchronise, the first `count` of them handed out.
int fetch_flat(cwslg_ctx *c, int ch_id, int k, int long_list, void *dst, size_t item, int max, int *n, uint64_t *start_epoch)
{
    if (!c || !n || (max > 0 && !dst)) return CWSLG_ERR_ARG;
    *n = 0;
    RecSource s;
    ResultFetch rf;                     // ticket + lifetime, released when the copy is done or the call fails
    const int rc = fetch_begin(c, ch_id, k, long_list, start_epoch, s, rf);
    if (rc) return rc;
    // no context lock from here on
    const int lim = std::min(std::max(max, 0), s.cap);
    int cnt = 0;
    std::vector<char> tmp((size_t)lim * item);
    HIPCHK(c, hipStreamWaitEvent(rf.fs, rf.ev, 0));
    HIPCHK(c, hipMemcpyAsync(&cnt, s.cnt, sizeof(int), hipMemcpyDeviceToHost, rf.fs));
    if (lim > 0) HIPCHK(c, hipMemcpyAsync(tmp.data(), s.rec, tmp.size(), hipMemcpyDeviceToHost, rf.fs));
    HIPCHK(c, hipStreamSynchronize(rf.fs));
    cnt = std::max(0, std::min(cnt, lim));
    if (cnt > 0) std::memcpy(dst, tmp.data(), (size_t)cnt * item);
    *n = cnt;
    return CWSLG_OK;
}

// The FT4 chain's slot layout rec[cnt][3] with nrec[k] records of candidate k, compacted in candidate order, then segment order (entry q of one
// kind belongs to entry q of every other).  At most `max` items are written; the return value counts them all.
int compact_records(void *dst, size_t item, int max, const int *nrec, const char *rec, int cnt)
{
    int out = 0;
    for (int k = 0; k < cnt; ++k)
        for (int q = 0; q < nrec[k] && q < 3; ++q) {
            if (out < max) std::memcpy((char *)dst + (size_t)out * item, rec + ((size_t)k * 3 + q) * item, item);
            ++out;
        }
    return out;
}

// Walk body: the count, synchronise, then nrec[count] and rec[count][3], synchronise, compacted.  An empty list is CWSLG_OK with the epoch set
// and no second copy.
int fetch_walk(cwslg_ctx *c, int ch_id, int k, void *dst, size_t item, int max, int *n, uint64_t *start_epoch)
{
    if (!c || !n || (max > 0 && !dst)) return CWSLG_ERR_ARG;
    *n = 0;
    RecSource s;
    ResultFetch rf;
    const int rc = fetch_begin(c, ch_id, k, 0, start_epoch, s, rf);
    if (rc) return rc;
    int cnt = 0;
    HIPCHK(c, hipStreamWaitEvent(rf.fs, rf.ev, 0));
    HIPCHK(c, hipMemcpyAsync(&cnt, s.cnt, sizeof(int), hipMemcpyDeviceToHost, rf.fs));
    HIPCHK(c, hipStreamSynchronize(rf.fs));
    cnt = std::max(0, std::min(cnt, s.cap));
    if (cnt <= 0) return CWSLG_OK;
    std::vector<int> nrec((size_t)cnt);
    std::vector<char> rec((size_t)cnt * 3 * item);
    HIPCHK(c, hipMemcpyAsync(nrec.data(), s.nrec, nrec.size() * sizeof(int), hipMemcpyDeviceToHost, rf.fs));
    HIPCHK(c, hipMemcpyAsync(rec.data(), s.rec, rec.size(), hipMemcpyDeviceToHost, rf.fs));
    HIPCHK(c, hipStreamSynchronize(rf.fs));
    *n = std::min(compact_records(dst, item, max, nrec.data(), rec.data(), cnt), max);
    return CWSLG_OK;
}

} // namespace

extern "C" {

int cwslg_enable_sync(cwslg_ctx *c, int enable, float syncmin, int max_cand, int f_lo_hz, int f_hi_hz)
{
    if (!c) return CWSLG_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    if (enable) {
        if (max_cand < 1 || max_cand > SYNC_MAXCAND_CAP || f_lo_hz < 0 || f_hi_hz <= f_lo_hz || f_hi_hz > 6000)
            return fail(c, CWSLG_ERR_ARG, "sync parameters out of range");
        const float df = 12000.0f / 3840.0f;
        SyncConfig cfg;
        cfg.enabled = true; cfg.syncmin = syncmin; cfg.max_cand = max_cand; cfg.f_lo_hz = f_lo_hz; cfg.f_hi_hz = f_hi_hz;
        cfg.ia = std::max(1, (int)std::lround((float)f_lo_hz / df));          // sync8: ia=max(1,nint(nfa/df))
        cfg.ib = (int)std::lround((float)f_hi_hz / df);                       //        ib=nint(nfb/df)
        if (cfg.ib + 12 > FT8_NH1) cfg.ib = FT8_NH1 - 12;
        if (cfg.ib < cfg.ia) return fail(c, CWSLG_ERR_ARG, "empty sync frequency range");
        cfg.nbins = (cfg.ib + 13 + 31) / 32 * 32;   // row pitch = whole 128-byte lines (ft8_sync_chan_kernel fetches one line per band and step)
        // the chains' settings, the coherent stage and the list order survive a re-enable.  syncmin_ft4 does NOT: it falls back to its default,
        // and every caller sets it again behind this call ("cwslg_enable_sync starts from the default threshold": tests/test_gpu_ft4_decode.py,
        // test_gpu_ft4_osd.py, test_gpu_record_fetch_races.py)
        cfg.kept = c->sync_cfg.kept;
        if (cfg.kept.ft8_soft) cfg.nbins = (cfg.ib + 15 + 31) / 32 * 32;   // soft bits on: tone 7 of bin ib (ib + 14) lies inside the row
        hipSetDevice(c->device);
        const int rc = sync_ensure_shared(c);             // the stage is enabled only with its tables in place
        if (rc) { c->sync_cfg.enabled = false; return rc; }
        c->sync_cfg = cfg;
        return CWSLG_OK;
    }
    c->sync_cfg.enabled = false;
    return CWSLG_OK;
}

int cwslg_set_candidate_order(cwslg_ctx *c, int order)
{
    if (!c || (order != CWSLG_ORDER_SYNC_DESC && order != CWSLG_ORDER_FREQ_ASC)) return CWSLG_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    c->sync_cfg.kept.order = order;
    return CWSLG_OK;
}

int cwslg_set_ft4_syncmin(cwslg_ctx *c, float syncmin)
{
    if (!c) return CWSLG_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    c->sync_cfg.syncmin_ft4 = syncmin;
    return CWSLG_OK;
}

// The list of an FT8 or FT4 channel; it survives a boundary that ran with the stage disabled, under its own epoch.
int cwslg_fetch_candidates(cwslg_ctx *c, int ch_id, cwslg_candidate *dst, int max, int *n, uint64_t *start_epoch)
{
    static_assert(sizeof(cwslg_candidate) == sizeof(SyncChannelBuffers::Cand), "candidate layout");
    return fetch_flat(c, ch_id, REC_CAND, 0, dst, sizeof(cwslg_candidate), max, n, start_epoch);
}

// FT8 soft bits (ft8soft_kernels.hpp).  The records are handed out like the lists, and only together with them: a fetch needs the records, the
// list and the frame to be of ONE epoch (the REC_SOFT8 row of record_kinds.hpp) -- after a boundary that ran with the feature off there is nothing to
// fetch, never an older slot's records under the newer epoch.
int cwslg_enable_ft8_softbits(cwslg_ctx *c, int enable)
{
    if (!c) return CWSLG_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    if (enable && !c->sync_cfg.enabled) return fail(c, CWSLG_ERR_ARG, "FT8 soft bits need the sync stage (cwslg_enable_sync)");
    SyncConfig &cfg = c->sync_cfg;
    cfg.kept.ft8_soft = enable != 0;
    // the row pitch: ib + 13 as ever while the feature is off; ib + 15 while it is on (channels reallocate at their next boundary)
    cfg.nbins = (cfg.ib + (cfg.kept.ft8_soft ? 15 : 13) + 31) / 32 * 32;
    return CWSLG_OK;
}

int cwslg_fetch_ft8_softbits(cwslg_ctx *c, int ch_id, cwslg_ft8_soft *dst, int max, int *n, uint64_t *start_epoch)
{
    static_assert(sizeof(cwslg_ft8_soft) == sizeof(Ft8SoftRec), "record layout");
    return fetch_flat(c, ch_id, REC_SOFT8, 0, dst, sizeof(cwslg_ft8_soft), max, n, start_epoch);
}

// The generator's device block exists from the first use of OSD on (while OSD has never been used a context holds no byte of it).
hipError_t osd_upload_gen(cwslg_ctx *c)
{
    SyncShared &s = c->sync_shared;
    hipError_t e = hipSuccess;
    if (!s.d_osdgen && (e = hipMalloc(&s.d_osdgen, sizeof(OsdGen))) != hipSuccess) return e;
    if (!s.osd_dirty) return hipSuccess;
    if ((e = sync_streams(c)) != hipSuccess) return e;
    if ((e = hipMemcpy(s.d_osdgen, s.osd_gen, sizeof(OsdGen), hipMemcpyHostToDevice)) != hipSuccess) return e;
    s.osd_dirty = false;
    return hipSuccess;
}

// FT8 decode (ldpc_kernels.hpp).  The parity-check table is the caller's data: validated and turned into the kernel's tables on the host
// (ldpc_host.hpp), uploaded with the context's streams drained -- a new table applies to every launch queued after the call.
int cwslg_set_ldpc_code(cwslg_ctx *c, const uint8_t *nm)
{
    if (!c || !nm) return CWSLG_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    LdpcTables t;
    const int why = ldpc_derive(nm, &t);
    if (why) {
        static const char *const reason[] = {"", "a position above 174", "a zero that is not the last entry of its row", "a position twice in one row",
                                             "a position that does not occur exactly three times"};
        return fail(c, CWSLG_ERR_ARG, "LDPC table rejected: %s", reason[why]);
    }
    // OSD's generator of the same code (osd_kernels.hpp); a table whose H has rank below 83 is still a code the BP decode takes, but OSD cannot
    // run on it: loading one switches OSD off
    OsdGen gen;
    const bool full_rank = ldpc_generator(t, &gen) == LDPC_M;
    hipSetDevice(c->device);
    if (!c->sync_shared.d_ldpc) HIPCHK(c, hipMalloc(&c->sync_shared.d_ldpc, sizeof(LdpcTables)));
    HIPCHK(c, sync_streams(c));                                // no queued decode launch may still read the old tables
    HIPCHK(c, hipMemcpy(c->sync_shared.d_ldpc, &t, sizeof(LdpcTables), hipMemcpyHostToDevice));
    static_assert(sizeof(c->sync_shared.ldpc_tables) == sizeof(LdpcTables), "table block");
    std::memcpy(c->sync_shared.ldpc_tables, &t, sizeof(LdpcTables));
    c->sync_shared.ldpc_loaded = true;
    c->sync_shared.osd_ready = false;
    // the systematic encoder of the decode reports: host bytes only (the device copy is made by the first cwslg_fetch_decode_reports after this
    // load); a table whose columns 91..173 are singular is still a code the decoders take, it merely has no reports
    {
        OsdGen enc;
        c->sync_shared.enc_ready = ldpc_encoder(t, &enc);
        c->sync_shared.enc_dirty = c->sync_shared.enc_ready;
        static_assert(sizeof(c->sync_shared.enc_gen) == sizeof(OsdGen), "encoder block");
        if (c->sync_shared.enc_ready) std::memcpy(c->sync_shared.enc_gen, &enc, sizeof(OsdGen));
    }
    if (full_rank) {
        static_assert(sizeof(c->sync_shared.osd_gen) == sizeof(OsdGen), "generator block");
        std::memcpy(c->sync_shared.osd_gen, &gen, sizeof(OsdGen));
        c->sync_shared.osd_ready = c->sync_shared.osd_dirty = true;
        if (c->sync_shared.d_osdgen) HIPCHK(c, osd_upload_gen(c));      // (the streams are drained: no queued OSD launch still reads the old block)
    } else {
        c->sync_cfg.kept.ft8_osd = false;
        c->sync_cfg.kept.ft4_osd = false;
    }
    return CWSLG_OK;
}

int cwslg_enable_ft8_decode(cwslg_ctx *c, int enable, int max_iter, int min_nsync)
{
    if (!c) return CWSLG_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    SyncConfig &cfg = c->sync_cfg;
    if (!enable) { cfg.kept.ft8_decode = false; return CWSLG_OK; }
    if (max_iter < 1 || max_iter > 200 || min_nsync < 0 || min_nsync > 22) return fail(c, CWSLG_ERR_ARG, "FT8 decode parameters out of range");
    if (!c->sync_shared.ldpc_loaded) return fail(c, CWSLG_ERR_ARG, "FT8 decode needs a parity-check table (cwslg_set_ldpc_code)");
    if (!cfg.enabled || !cfg.kept.ft8_soft) return fail(c, CWSLG_ERR_ARG, "FT8 decode needs the sync stage and FT8 soft bits (cwslg_enable_sync, cwslg_enable_ft8_softbits)");
    cfg.kept.ft8_decode = true; cfg.kept.ldpc_max_iter = max_iter; cfg.kept.ldpc_min_nsync = min_nsync;
    return CWSLG_OK;
}

// Handed out like the soft-bit records, and only together with them: decode records, soft-bit records, list and frame of ONE epoch.
int cwslg_fetch_ft8_decode(cwslg_ctx *c, int ch_id, cwslg_ft8_msg *dst, int max, int *n, uint64_t *start_epoch)
{
    static_assert(sizeof(cwslg_ft8_msg) == sizeof(Ft8MsgRec), "record layout");
    return fetch_flat(c, ch_id, REC_MSG8, 0, dst, sizeof(cwslg_ft8_msg), max, n, start_epoch);
}

// The same kernel on n sets of 174 metrics from host memory, no nsync filter; synchronous (temporary device buffers, the context's stream).
int cwslg_ldpc_decode(cwslg_ctx *c, const float *llr, int n, int max_iter, cwslg_ft8_msg *out)
{
    if (!c || n < 0 || (n > 0 && (!llr || !out))) return CWSLG_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    if (max_iter < 1 || max_iter > 200) return fail(c, CWSLG_ERR_ARG, "max_iter out of range (1..200)");
    if (!c->sync_shared.ldpc_loaded) return fail(c, CWSLG_ERR_ARG, "no parity-check table loaded (cwslg_set_ldpc_code)");
    if (n == 0) return CWSLG_OK;
    hipSetDevice(c->device);
    const size_t in_bytes = (size_t)n * LDPC_N * sizeof(float), out_bytes = (size_t)n * sizeof(Ft8MsgRec);
    char *d = nullptr;
    HIPCHK(c, hipMalloc((void **)&d, in_bytes + out_bytes));      // (in_bytes is a multiple of 8: the records behind it are aligned)
    hipError_t e = hipMemcpyAsync(d, llr, in_bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        ldpc_launch_flat(c->stream, c->sync_shared.d_ldpc, (const float *)d, (Ft8MsgRec *)(d + in_bytes), n, max_iter);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d + in_bytes, out_bytes, hipMemcpyDeviceToHost, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(c, CWSLG_ERR_HIP, "cwslg_ldpc_decode failed: %s", hipGetErrorString(e));
    return CWSLG_OK;
}

// FT8 OSD (osd_kernels.hpp): one launch behind the decode launch, on the candidates it attempted without crc_ok.
int cwslg_enable_ft8_osd(cwslg_ctx *c, int enable, int order, int min_nsync)
{
    if (!c) return CWSLG_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    SyncConfig &cfg = c->sync_cfg;
    if (!enable) { cfg.kept.ft8_osd = false; return CWSLG_OK; }
    if (order < 0 || order > 2 || min_nsync < 0 || min_nsync > 22) return fail(c, CWSLG_ERR_ARG, "FT8 OSD parameters out of range");
    if (!c->sync_shared.osd_ready) return fail(c, CWSLG_ERR_ARG, "FT8 OSD needs a parity-check table of rank 83 (cwslg_set_ldpc_code)");
    hipSetDevice(c->device);
    HIPCHK(c, osd_upload_gen(c));
    cfg.kept.ft8_osd = true; cfg.kept.osd_order = order; cfg.kept.osd_min_nsync = min_nsync;
    return CWSLG_OK;
}

// Handed out like the decode records, and only together with them: OSD, decode and soft-bit records, list and frame of ONE epoch.
int cwslg_fetch_ft8_osd(cwslg_ctx *c, int ch_id, cwslg_osd_msg *dst, int max, int *n, uint64_t *start_epoch)
{
    static_assert(sizeof(cwslg_osd_msg) == sizeof(OsdRec), "record layout");
    return fetch_flat(c, ch_id, REC_OSD8, 0, dst, sizeof(cwslg_osd_msg), max, n, start_epoch);
}

// The same kernel on n sets of 174 metrics from host memory, no gates; synchronous (temporary device buffers, the context's stream).
int cwslg_osd_decode(cwslg_ctx *c, const float *llr, int n, int order, cwslg_osd_msg *out)
{
    if (!c || n < 0 || (n > 0 && (!llr || !out))) return CWSLG_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    if (order < 0 || order > 2) return fail(c, CWSLG_ERR_ARG, "order out of range (0..2)");
    if (!c->sync_shared.osd_ready) return fail(c, CWSLG_ERR_ARG, "no parity-check table of rank 83 loaded (cwslg_set_ldpc_code)");
    if (n == 0) return CWSLG_OK;
    hipSetDevice(c->device);
    HIPCHK(c, osd_upload_gen(c));
    const size_t in_bytes = (size_t)n * LDPC_N * sizeof(float), out_bytes = (size_t)n * sizeof(OsdRec);
    char *d = nullptr;
    HIPCHK(c, hipMalloc((void **)&d, in_bytes + out_bytes));      // (in_bytes is a multiple of 8: the records behind it are aligned)
    hipError_t e = hipMemcpyAsync(d, llr, in_bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        osd_launch_flat(c->stream, c->sync_shared.d_osdgen, (const float *)d, (OsdRec *)(d + in_bytes), n, order);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d + in_bytes, out_bytes, hipMemcpyDeviceToHost, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(c, CWSLG_ERR_HIP, "cwslg_osd_decode failed: %s", hipGetErrorString(e));
    return CWSLG_OK;
}

// FT8 a-priori decoding (ap_kernels.hpp).  The patterns are the caller's data: validated and packed on the host (ap_host.hpp), host bytes only --
// every AP call takes the block in force at the call up with its own upload, so nothing queued ever reads a block that a later set replaces.
static int set_ap_impl(cwslg_ctx *c, const cwslg_ap_pattern *pat, int n_pat, int max_iter, int min_nsync, int min_nqual, bool ft4)
{
    static_assert(sizeof(cwslg_ap_pattern) == sizeof(ApPattern), "pattern layout");
    if (!c) return CWSLG_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    if (max_iter < 1 || max_iter > 200 || min_nsync < 0 || min_nsync > (ft4 ? 17 : 22) || min_nqual < 0 || min_nqual > 33)
        return fail(c, CWSLG_ERR_ARG, "%s AP parameters out of range", ft4 ? "FT4" : "FT8");
    ApBlock b;
    const int why = ap_pack(reinterpret_cast<const ApPattern *>(pat), n_pat, &b);
    if (why) {
        static const char *const reason[] = {"", "n_pat outside 0..8, or no pattern array", "a mask or value bit at position 91..95", "a value bit outside its mask"};
        return fail(c, CWSLG_ERR_ARG, "AP patterns rejected: %s", reason[why]);
    }
    SyncShared &s = c->sync_shared;
    static_assert(sizeof(s.ap_block) == sizeof(ApBlock) && sizeof(s.ap4_block) == sizeof(ApBlock), "pattern block");
    if (ft4) {
        std::memcpy(s.ap4_block, &b, sizeof(ApBlock));
        s.ap4_npat = n_pat; s.ap4_max_iter = max_iter; s.ap4_min_nsync = min_nsync; s.ap4_min_nqual = min_nqual;
    } else {
        std::memcpy(s.ap_block, &b, sizeof(ApBlock));
        s.ap_npat = n_pat; s.ap_max_iter = max_iter; s.ap_min_nsync = min_nsync;
    }
    return CWSLG_OK;
}

int cwslg_set_ft8_ap(cwslg_ctx *c, const cwslg_ap_pattern *pat, int n_pat, int max_iter, int min_nsync)
{
    return set_ap_impl(c, pat, n_pat, max_iter, min_nsync, 0, false);
}

// The FT4 patterns: a state of their own beside the FT8 one (the same validation, cwslg_enable_ft4_decode's ranges for the two minima).
int cwslg_set_ft4_ap(cwslg_ctx *c, const cwslg_ap_pattern *pat, int n_pat, int max_iter, int min_nsync, int min_nqual)
{
    return set_ap_impl(c, pat, n_pat, max_iter, min_nsync, min_nqual, true);
}

// The a-priori decode (ap_kernels.hpp: ap_decode_kernel) on n sets of 174 metrics from host memory, no gate; synchronous (temporary device buffers, the context's stream).  The
// patterns and the tables of the code go up in front of the metrics: in | pattern block | tables | metrics | records.
int cwslg_ap_decode(cwslg_ctx *c, const float *llr, int n, cwslg_ap_msg *out)
{
    static_assert(sizeof(cwslg_ap_msg) == sizeof(ApMsgRec), "record layout");
    if (!c || n < 0 || (n > 0 && (!llr || !out))) return CWSLG_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    const SyncShared &s = c->sync_shared;
    if (!s.ldpc_loaded) return fail(c, CWSLG_ERR_ARG, "no parity-check table loaded (cwslg_set_ldpc_code)");
    if (s.ap_npat <= 0) return fail(c, CWSLG_ERR_ARG, "no AP pattern set (cwslg_set_ft8_ap)");
    if (n == 0) return CWSLG_OK;
    hipSetDevice(c->device);
    const size_t pat_at = 0, tab_at = 256, llr_at = tab_at + sizeof(LdpcTables);
    const size_t in_bytes = (size_t)n * LDPC_N * sizeof(float), out_at = llr_at + in_bytes, out_bytes = (size_t)n * sizeof(ApMsgRec);
    char *d = nullptr;
    HIPCHK(c, hipMalloc((void **)&d, out_at + out_bytes));      // (every part starts at a multiple of 8)
    hipError_t e = hipMemcpyAsync(d + pat_at, s.ap_block, sizeof(ApBlock), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d + tab_at, s.ldpc_tables, sizeof(LdpcTables), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d + llr_at, llr, in_bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        ap_launch_flat(c->stream, d + tab_at, d + pat_at, s.ap_npat, (const float *)(d + llr_at), (ApMsgRec *)(d + out_at), n, s.ap_max_iter);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d + out_at, out_bytes, hipMemcpyDeviceToHost, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(c, CWSLG_ERR_HIP, "cwslg_ap_decode failed: %s", hipGetErrorString(e));
    return CWSLG_OK;
}

int cwslg_enable_ft4_coherent(cwslg_ctx *c, int enable)
{
    if (!c) return CWSLG_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    c->sync_cfg.kept.ft4_coherent = enable != 0;
    return CWSLG_OK;
}

int cwslg_fetch_ft4_sync(cwslg_ctx *c, int ch_id, cwslg_ft4_sync *dst, int max, int *n, uint64_t *start_epoch)
{
    static_assert(sizeof(cwslg_ft4_sync) == sizeof(Ft4Rec), "record layout");
    return fetch_walk(c, ch_id, REC_FT4SYNC, dst, sizeof(cwslg_ft4_sync), max, n, start_epoch);
}

// FT4 soft bits (ft4soft_kernels.hpp).  One record per cwslg_ft4_sync record, compacted from the slot layout by the same nrec walk as
// cwslg_fetch_ft4_sync; handed out only when soft records, sync records, list and frame are of ONE epoch (the REC_SOFT4 row of record_kinds.hpp: the
// launch that sets its stamp runs behind the refinement of the same boundary) -- after a boundary that ran with the feature or the coherent stage
// off there is nothing to fetch, never an older slot's records under the newer epoch.
int cwslg_enable_ft4_softbits(cwslg_ctx *c, int enable)
{
    if (!c) return CWSLG_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    if (enable && !c->sync_cfg.enabled) return fail(c, CWSLG_ERR_ARG, "FT4 soft bits need the sync stage (cwslg_enable_sync)");
    c->sync_cfg.kept.ft4_soft = enable != 0;
    return CWSLG_OK;
}

int cwslg_fetch_ft4_softbits(cwslg_ctx *c, int ch_id, cwslg_ft4_soft *dst, int max, int *n, uint64_t *start_epoch)
{
    static_assert(sizeof(cwslg_ft4_soft) == sizeof(Ft4SoftRec), "record layout");
    return fetch_walk(c, ch_id, REC_SOFT4, dst, sizeof(cwslg_ft4_soft), max, n, start_epoch);
}

// FT4 decode (ldpc_kernels.hpp's third addressing mode): the FT8 decode's rules with the FT4 soft bits in the place of the FT8 ones.
int cwslg_enable_ft4_decode(cwslg_ctx *c, int enable, int max_iter, int min_nsync, int min_nqual)
{
    if (!c) return CWSLG_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    SyncConfig &cfg = c->sync_cfg;
    if (!enable) { cfg.kept.ft4_decode = false; return CWSLG_OK; }
    if (max_iter < 1 || max_iter > 200 || min_nsync < 0 || min_nsync > 17 || min_nqual < 0 || min_nqual > 33)
        return fail(c, CWSLG_ERR_ARG, "FT4 decode parameters out of range");
    if (!c->sync_shared.ldpc_loaded) return fail(c, CWSLG_ERR_ARG, "FT4 decode needs a parity-check table (cwslg_set_ldpc_code)");
    if (!cfg.enabled || !cfg.kept.ft4_soft) return fail(c, CWSLG_ERR_ARG, "FT4 decode needs the sync stage and FT4 soft bits (cwslg_enable_sync, cwslg_enable_ft4_softbits)");
    cfg.kept.ft4_decode = true; cfg.kept.ldpc4_max_iter = max_iter; cfg.kept.ldpc4_min_nsync = min_nsync; cfg.kept.ldpc4_min_nqual = min_nqual;
    return CWSLG_OK;
}

// Handed out like the FT4 soft-bit records (the same nrec walk over the same slot layout), and only together with them: decode records, soft
// records, sync records, list and frame of ONE epoch.
int cwslg_fetch_ft4_decode(cwslg_ctx *c, int ch_id, cwslg_ft4_msg *dst, int max, int *n, uint64_t *start_epoch)
{
    static_assert(sizeof(cwslg_ft4_msg) == sizeof(Ft4MsgRec), "record layout");
    return fetch_walk(c, ch_id, REC_MSG4, dst, sizeof(cwslg_ft4_msg), max, n, start_epoch);
}

// FT4 OSD (osd_kernels.hpp's third addressing mode): one launch behind the FT4 decode launch, on the sets of the records no set of which BP
// brought to crc_ok.
int cwslg_enable_ft4_osd(cwslg_ctx *c, int enable, int order, int min_nsync, int min_nqual)
{
    if (!c) return CWSLG_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    SyncConfig &cfg = c->sync_cfg;
    if (!enable) { cfg.kept.ft4_osd = false; return CWSLG_OK; }
    if (order < 0 || order > 2 || min_nsync < 0 || min_nsync > 17 || min_nqual < 0 || min_nqual > 33)
        return fail(c, CWSLG_ERR_ARG, "FT4 OSD parameters out of range");
    if (!c->sync_shared.osd_ready) return fail(c, CWSLG_ERR_ARG, "FT4 OSD needs a parity-check table of rank 83 (cwslg_set_ldpc_code)");
    hipSetDevice(c->device);
    HIPCHK(c, osd_upload_gen(c));
    cfg.kept.ft4_osd = true; cfg.kept.osd4_order = order; cfg.kept.osd4_min_nsync = min_nsync; cfg.kept.osd4_min_nqual = min_nqual;
    return CWSLG_OK;
}

// Handed out like the FT4 decode records (the same nrec walk over the same slot layout), and only together with them: OSD, decode and soft
// records, sync records, list and frame of ONE epoch.
int cwslg_fetch_ft4_osd(cwslg_ctx *c, int ch_id, cwslg_ft4_osd *dst, int max, int *n, uint64_t *start_epoch)
{
    static_assert(sizeof(cwslg_ft4_osd) == sizeof(Ft4OsdRec), "record layout");
    return fetch_walk(c, ch_id, REC_OSD4, dst, sizeof(cwslg_ft4_osd), max, n, start_epoch);
}

// The decoded words of a whole FT8 / FT4 group (harvest_kernels.hpp; the contract is the header's).  A fetch like the others -- pointers read
// under the context mutex, one ticket of the group, the work on a fetch stream behind the group's generation event with the mutex released --
// except that what runs on the fetch stream is a descriptor upload, decode_harvest_kernel (count, scan, emit) and ONE copy down.  It writes only
// the group's HarvestStage: no record, list, stamp or statistic changes.
// reports (cwslg_fetch_decode_reports for FT8, cwslg_fetch_ft4_decode_reports for FT4): a ReportDesc / Ft4ReportDesc per channel goes up behind
// the HarvestDesc array in the same copy, ONE further launch (report_launch / ft4_report_launch) follows the three, and the reports come down
// behind the records in the same copy.
// FT4: a channel takes part only if its REC_MSG4 epoch is the frame's epoch, so sync_launch queued REC_MSG4 for that frame at the last boundary;
// records_queued queues it only behind REC_SOFT4 and REC_FT4SYNC, i.e. with ft4_coherent on in the configuration of that boundary -- the same
// switch under which sync_launch runs ft4_dft567 / ft4_fft64_unpack on the channel's Ft4Work (cx = d_cx).  d_cx therefore holds THAT frame's
// spectrum, and the sync records read here are that boundary's too: no path hands a stale spectrum to the report.
// a-priori (cwslg_fetch_ft8_ap, cwslg_fetch_ft4_ap; ap_kernels.hpp): an ApDesc per channel, the pattern block and the tables of the code in force go up
// behind the HarvestDesc array in the same copy; the a-priori decode (ap_decode_kernel) runs IN FRONT of the three harvest launches and leaves a decode-record array
// per channel in the group's AP staging, which is what HarvestDesc.msg then points at (.osd null); one annotate launch follows them.
// subtraction (cwslg_subtract_ft8, cwslg_subtract_ft4; ft8sub_host.inc, modules/ft8sub.hip, modules/ft4sub.hip): a SubDesc per channel goes up like the ReportDesc, the head comes down behind
// the harvest launches (the fit records are sized by what was emitted), the module's fit and apply launches follow, and the 28-byte reports come
// down behind the records in the same copy; the residuals stay on the device, in the group's block.
enum { FETCH_DECODES = 0, FETCH_REPORTS = 1, FETCH_AP = 2, FETCH_SUBTRACT = 3 };
static int fetch_decodes_impl(cwslg_ctx *c, int group, uint64_t *start_epoch, cwslg_decode *dst, cwslg_decode_report *rep, int max, int *n, int *n_total,
                              int *n_channels, int what, cwslg_subtract_report *sub = nullptr)
{
    const bool subtract = what == FETCH_SUBTRACT;
    const bool reports = what == FETCH_REPORTS || subtract, ap = what == FETCH_AP;      // (subtract: the reports' encoder, serialisation and block layout)
    static_assert(sizeof(cwslg_subtract_report) == F8SUB_REP_WORDS * sizeof(unsigned), "record layout");
    const size_t rep_words = subtract ? F8SUB_REP_WORDS : REPORT_WORDS;
    std::vector<SubDesc> sdescs;
    std::vector<int> sub_chans;
    // (subtract: the group's own stage, frame length, fit record and tiling -- FT8 180000 samples, FT4 the decoder's first 72576)
    Ft8SubStage &sub_stage = group == CWSLG_GROUP_FT4 ? c->ft4sub : c->ft8sub;
    const size_t sub_n = group == CWSLG_GROUP_FT4 ? F4SUB_N : F8SUB_N, sub_rec_words = group == CWSLG_GROUP_FT4 ? F4SUB_REC_WORDS : F8SUB_REC_WORDS;
    static_assert(sizeof(cwslg_decode) == HARVEST_REC_WORDS * sizeof(unsigned), "record layout");
    static_assert(sizeof(cwslg_decode_report) == sizeof(ReportRec), "record layout");
    const bool ft4 = group == CWSLG_GROUP_FT4;
    const int k_msg = ft4 ? REC_MSG4 : REC_MSG8, k_osd = ft4 ? REC_OSD4 : REC_OSD8;
    HarvestStage &hs = c->harvest[ft4 ? 1 : 0];
    std::lock_guard<std::mutex> serial(hs.mu);
    std::unique_lock<std::mutex> report_serial;     // reports: also against the other group's report calls, from the encoder's upload to the synchronise
    if (reports) report_serial = std::unique_lock<std::mutex>(c->report_mu);
    std::vector<HarvestDesc> descs;
    std::vector<ReportDesc> rdescs;
    std::vector<Ft4ReportDesc> rdescs4;
    std::vector<ApDesc> adescs;
    ApBlock ap_block{};
    LdpcTables ap_tables{};
    int ap_npat = 0, ap_max_iter = 0, ap_min_nsync = 0, ap_min_nqual = 0, ap_cap_max = 0;
    // AP staging per entry slot: FT8 a 20-byte record and its dmin; FT4 three slots per candidate, each a 60-byte record and three dmin
    const size_t ap_per_cand = ft4 ? 3 * (sizeof(Ft4MsgRec) + 3 * sizeof(float)) : sizeof(Ft8MsgRec) + sizeof(float);
    Ft4Tables tb4{};
    const float2 *d_w32 = nullptr;
    const uint32_t *d_enc = nullptr;
    size_t bound = 0;                   // no more decodes than entries
    ResultFetch rf;                     // ticket + lifetime, released when the copy is done or the call fails
    {
        std::lock_guard<std::mutex> g(c->mu);
        if (subtract) {
            const uint32_t *unused = nullptr;
            hipSetDevice(c->device);
            int rc = ft8sub_encoder(c, &unused);        // (the code first: a table without systematic form is CWSLG_ERR_ARG whatever else is there)
            if (!rc) rc = group == CWSLG_GROUP_FT4 ? ft4sub_module(c) : ft8sub_module(c);
            if (rc) return rc;
        }
        if (reports && !c->sync_shared.enc_ready)
            return fail(c, CWSLG_ERR_ARG, "%s", c->sync_shared.ldpc_loaded ? "decode reports need a systematic code: columns 91..173 of the loaded parity-check table are singular"
                                                                    : "decode reports need a parity-check table (cwslg_set_ldpc_code)");
        if (ap) {
            const SyncShared &s = c->sync_shared;
            if (!s.ldpc_loaded) return fail(c, CWSLG_ERR_ARG, "a-priori decoding needs a parity-check table (cwslg_set_ldpc_code)");
            if ((ft4 ? s.ap4_npat : s.ap_npat) <= 0) return fail(c, CWSLG_ERR_ARG, "no AP pattern set (%s)", ft4 ? "cwslg_set_ft4_ap" : "cwslg_set_ft8_ap");
            std::memcpy(&ap_block, ft4 ? s.ap4_block : s.ap_block, sizeof(ApBlock));
            std::memcpy(&ap_tables, s.ldpc_tables, sizeof(LdpcTables));
            ap_npat = ft4 ? s.ap4_npat : s.ap_npat; ap_max_iter = ft4 ? s.ap4_max_iter : s.ap_max_iter;
            ap_min_nsync = ft4 ? s.ap4_min_nsync : s.ap_min_nsync; ap_min_nqual = ft4 ? s.ap4_min_nqual : 0;
        }
        uint64_t E = *start_epoch;
        std::vector<std::pair<int, uint64_t>> live;
        for (size_t id = 0; id < c->chans.size(); ++id) {
            const Channel &ch = c->chans[id];
            if (!ch.open || ch.group != group || !(ft4 ? ch.sync_ft4 : ch.sync_ft8)) continue;      // (a JS8 channel of the FT8 group has no chain)
            const uint64_t e = channel_records_epoch(ch, k_msg, ch.syncbuf.d_block);
            if (e) live.emplace_back((int)id, e);
        }
        if (!E) for (const auto &l : live) E = std::max(E, l.second);
        for (const auto &l : live) {
            if (l.second != E) continue;
            const Channel &ch = c->chans[l.first];
            const SyncChannelBuffers &b = ch.syncbuf;
            const bool osd = channel_records_epoch(ch, k_osd, b.d_block) == E;
            HarvestDesc d{};
            d.cnt = b.d_ncand;
            d.list = ft4 ? b.d_rec : (const void *)b.d_cand;
            d.nrec = ft4 ? b.d_nrec : nullptr;
            d.msg = record_array(b, k_msg);
            d.osd = osd ? record_array(b, k_osd) : nullptr;
            d.cap = std::min(b.max_cand, (int)SYNC_MAXCAND_CAP);
            d.ch_id = l.first;
            descs.push_back(d);
            bound += (size_t)d.cap * (ft4 ? 3 : 1);
            if (ap) {           // (the staging pointers are filled in below, once its size is known)
                ApDesc a{};
                a.cnt = b.d_ncand;
                a.soft = ft4 ? (const void *)b.d_ft4soft : (const void *)b.d_soft;
                a.msg = d.msg;
                a.osd = d.osd;
                a.nrec = d.nrec;
                a.cap = d.cap;
                adescs.push_back(a);
                ap_cap_max = std::max(ap_cap_max, d.cap);
            } else if (reports && ft4 && !subtract) {
                Ft4ReportDesc r{};
                r.cx = b.d_cx;
                r.rec = (const Ft4Rec *)b.d_rec;
                r.nrec = b.d_nrec;
                r.cnt = b.d_ncand;
                r.cap = d.cap;
                rdescs4.push_back(r);
            } else if (subtract) {
                // (the device frame is the reference's 20 s buffer; the decoder's frame, and the subtractor's, is its first 15 s -- FT4: 72576 samples)
                if (ch.frame_len < sub_n || ((uintptr_t)ch.d_frame[ch.frame_idx] & 15u))
                    return fail(c, CWSLG_ERR_ARG, "channel %d: the subtractor needs a 16-byte aligned frame of at least %d samples", l.first, (int)sub_n);
                SubDesc r{};
                r.frame = ch.d_frame[ch.frame_idx];
                r.n_valid = (int)std::min(ch.frame_valid, sub_n);
                sdescs.push_back(r);               // (.resid: below, once the block is there)
                sub_chans.push_back(l.first);
            } else if (reports) {
                ReportDesc r{};
                r.spectra = b.d_spectra;
                r.list = b.d_cand;
                r.nbins = b.nbins;
                rdescs.push_back(r);
            }
        }
        if (descs.empty()) return CWSLG_ERR_NO_FRAME;
        hipSetDevice(c->device);
        if (reports) {
            // the encoder's device copy, made by the first call after a (re)load.  The report launches of the two groups are its only readers; they
            // belong to calls that report_mu serialises and that synchronise before they return: none is in flight now
            SyncShared &s = c->sync_shared;
            if (!s.d_encgen) HIPCHK(c, hipMalloc(&s.d_encgen, sizeof(OsdGen)));
            if (s.enc_dirty) {
                HIPCHK(c, hipMemcpy(s.d_encgen, s.enc_gen, sizeof(OsdGen), hipMemcpyHostToDevice));
                s.enc_dirty = false;
            }
            d_enc = (const uint32_t *)s.d_encgen;
            tb4 = c->ft4_tables;            // (FT4: built by the boundary that made the records)
            d_w32 = s.ft4_w32;
        }
        if (subtract) {
            // the group's residual block, a frame per channel that takes part.  Only calls that hs.mu serialises and that synchronise before they
            // return write it, and the residual fetches take hs.mu: none is in flight now.  Its epoch is withdrawn until this call has succeeded
            Ft8SubStage &st = sub_stage;
            st.resid_epoch = 0;
            st.resid_chans.clear();
            const size_t need = sdescs.size() * sub_n * sizeof(float);
            if (st.resid_bytes < need) {
                if (st.d_resid) (void)hipFree(st.d_resid);
                st.d_resid = nullptr; st.resid_bytes = 0;
                HIPCHK(c, hipMalloc((void **)&st.d_resid, need));
                st.resid_bytes = need;
            }
            for (size_t i = 0; i < sdescs.size(); ++i) sdescs[i].resid = st.d_resid + i * sub_n;
        }
        if (ap) {
            // the group's AP staging: per channel cap records of 20 bytes (FT4: 3 cap of 60), then their dmin words (FT4: three per record),
            // each channel from a multiple of 16.  Only calls that hs.mu serialises and that synchronise before they return touch it: none is
            // in flight now
            size_t need = 0;
            for (const ApDesc &a : adescs) need += ((size_t)a.cap * ap_per_cand + 15) & ~size_t(15);
            if (hs.ap_bytes < need) {
                if (hs.d_ap) (void)hipFree(hs.d_ap);
                hs.d_ap = nullptr; hs.ap_bytes = 0;
                HIPCHK(c, hipMalloc((void **)&hs.d_ap, need + need / 2));
                hs.ap_bytes = need + need / 2;
            }
            size_t at = 0;
            for (size_t i = 0; i < adescs.size(); ++i) {
                ApDesc &a = adescs[i];
                a.ap = hs.d_ap + at;
                a.dmin = (float *)(hs.d_ap + at + (size_t)a.cap * (ft4 ? 3 * sizeof(Ft4MsgRec) : sizeof(Ft8MsgRec)));
                at += ((size_t)a.cap * ap_per_cand + 15) & ~size_t(15);
                descs[i].msg = a.ap;
                descs[i].osd = nullptr;
            }
        }
        *start_epoch = E;
        const int rc = begin_result_fetch(c, c->chans[descs[0].ch_id], rf);
        if (rc) return rc;
    }
    // no context lock from here on
    const size_t nch = descs.size(), lim = std::min((size_t)std::max(max, 0), bound);
    auto pad = [](size_t v) { return (v + 255) & ~size_t(255); };
    const size_t desc_bytes = nch * sizeof(HarvestDesc), cnt_bytes = pad(nch * sizeof(unsigned));
    const size_t rdesc_bytes = subtract ? sdescs.size() * sizeof(SubDesc) : ft4 ? rdescs4.size() * sizeof(Ft4ReportDesc) : rdescs.size() * sizeof(ReportDesc);
    // a-priori: | HarvestDesc | ApDesc | pattern block | tables |, each from a multiple of 256
    const size_t adesc_at = pad(desc_bytes), apat_at = adesc_at + pad(adescs.size() * sizeof(ApDesc)), atab_at = apat_at + pad(sizeof(ApBlock));
    const size_t up_bytes = ap ? atab_at + sizeof(LdpcTables) : reports ? pad(desc_bytes) + rdesc_bytes : desc_bytes, up_pad = pad(up_bytes);
    // down: head | lim records | (reports: from the next 16-byte boundary) lim reports
    const size_t rec_words = HARVEST_HEAD_WORDS + lim * HARVEST_REC_WORDS, rep_at = (rec_words + 3) & ~size_t(3);
    const size_t out_bytes = (reports ? rep_at + lim * rep_words : rec_words) * sizeof(unsigned);
    const size_t h_need = up_pad + out_bytes, d_need = up_pad + 2 * cnt_bytes + out_bytes;
    if (hs.h_bytes < h_need) {
        if (hs.h) (void)hipHostFree(hs.h);
        hs.h = nullptr; hs.h_bytes = 0;
        HIPCHK(c, hipHostMalloc((void **)&hs.h, pad(h_need + h_need / 2), hipHostMallocDefault));
        hs.h_bytes = pad(h_need + h_need / 2);
    }
    if (hs.d_bytes < d_need) {
        if (hs.d) (void)hipFree(hs.d);
        hs.d = nullptr; hs.d_bytes = 0;
        HIPCHK(c, hipMalloc((void **)&hs.d, pad(d_need + d_need / 2)));
        hs.d_bytes = pad(d_need + d_need / 2);
    }
    std::memcpy(hs.h, descs.data(), desc_bytes);
    if (reports) std::memcpy(hs.h + pad(desc_bytes), subtract ? (const void *)sdescs.data() : ft4 ? (const void *)rdescs4.data() : (const void *)rdescs.data(), rdesc_bytes);
    if (ap) {
        std::memcpy(hs.h + adesc_at, adescs.data(), adescs.size() * sizeof(ApDesc));
        std::memcpy(hs.h + apat_at, &ap_block, sizeof(ApBlock));
        std::memcpy(hs.h + atab_at, &ap_tables, sizeof(LdpcTables));
    }
    unsigned *h_out = (unsigned *)(hs.h + up_pad);
    const HarvestDesc *d_desc = (const HarvestDesc *)hs.d;
    unsigned *d_counts = (unsigned *)(hs.d + up_pad), *d_offsets = (unsigned *)(hs.d + up_pad + cnt_bytes);
    unsigned *d_out = (unsigned *)(hs.d + up_pad + 2 * cnt_bytes);
    HIPCHK(c, hipStreamWaitEvent(rf.fs, rf.ev, 0));
    HIPCHK(c, hipMemcpyAsync(hs.d, hs.h, up_bytes, hipMemcpyHostToDevice, rf.fs));
    if (ap) ap_launch_chain(rf.fs, (const ApDesc *)(hs.d + adesc_at), (int)nch, ap_cap_max, ap_max_iter, ap_min_nsync, hs.d + atab_at, hs.d + apat_at, ap_npat, ft4, ap_min_nqual);
    harvest_launch(rf.fs, d_desc, d_counts, d_offsets, d_out, (int)nch, (int)lim, ft4 ? 1 : 0);
    if (ap) ap_launch_annotate(rf.fs, (const ApDesc *)(hs.d + adesc_at), d_offsets, d_out, (int)nch, (int)lim, ft4);
    if (subtract) {
        // what was emitted decides the size of the fit records: the head comes down first
        Ft8SubStage &st = sub_stage;
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(h_out, d_out, HARVEST_HEAD_WORDS * sizeof(unsigned), hipMemcpyDeviceToHost, rf.fs));
        HIPCHK(c, hipStreamSynchronize(rf.fs));
        const size_t n_emit = std::min((size_t)h_out[0], lim), need = n_emit * sub_rec_words * sizeof(unsigned);
        if (st.recs_bytes < need) {
            if (st.d_recs) (void)hipFree(st.d_recs);
            st.d_recs = nullptr; st.recs_bytes = 0;
            HIPCHK(c, hipMalloc((void **)&st.d_recs, need + need / 2));
            st.recs_bytes = need + need / 2;
        }
        HIPCHK(c, ft8sub_launch(st.fit, st.apply, rf.fs, (const SubDesc *)(hs.d + pad(desc_bytes)), d_offsets, d_out, d_enc, (unsigned *)st.d_recs, d_out + rep_at,
                                (int)nch, (int)n_emit, (int)lim, ft4 ? F4SUB_NTILE : F8SUB_NTILE));
    } else if (reports && ft4)
        ft4_report_launch(rf.fs, (const Ft4ReportDesc *)(hs.d + pad(desc_bytes)), d_offsets, d_out, d_enc, d_out + rep_at, tb4, d_w32, (int)nch, (int)lim);
    else if (reports)
        report_launch(rf.fs, (const ReportDesc *)(hs.d + pad(desc_bytes)), d_offsets, d_out, d_enc, d_out + rep_at, (int)nch, (int)lim);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_out, d_out, out_bytes, hipMemcpyDeviceToHost, rf.fs));
    HIPCHK(c, hipStreamSynchronize(rf.fs));
    const size_t total = h_out[0], got = std::min(total, lim);
    if (got && dst) std::memcpy(dst, h_out + HARVEST_HEAD_WORDS, got * sizeof(cwslg_decode));
    if (got && rep) std::memcpy(rep, h_out + rep_at, got * sizeof(cwslg_decode_report));
    if (got && sub) std::memcpy(sub, h_out + rep_at, got * sizeof(cwslg_subtract_report));
    if (subtract) {
        sub_stage.resid_chans = sub_chans;
        sub_stage.resid_epoch = *start_epoch;
    }
    *n = (int)got;
    *n_total = (int)total;
    if (n_channels) *n_channels = (int)nch;
    return CWSLG_OK;
}

int cwslg_fetch_decodes(cwslg_ctx *c, int group, uint64_t *start_epoch, cwslg_decode *dst, int max, int *n, int *n_total, int *n_channels)
{
    if (n) *n = 0;
    if (n_total) *n_total = 0;
    if (n_channels) *n_channels = 0;
    if (!c || !start_epoch || !n || !n_total || (max > 0 && !dst)) return CWSLG_ERR_ARG;
    if (group != CWSLG_GROUP_FT8 && group != CWSLG_GROUP_FT4) return fail(c, CWSLG_ERR_ARG, "decodes exist for the FT8 and FT4 groups only (group %d)", group);
    return fetch_decodes_impl(c, group, start_epoch, dst, nullptr, max, n, n_total, n_channels, FETCH_DECODES);
}

// The same call with a signal report per decode (harvest_kernels.hpp: decode_report_kernel; the contract is the header's, cwslg_decode_report).
int cwslg_fetch_decode_reports(cwslg_ctx *c, int group, uint64_t *start_epoch, cwslg_decode *dec, cwslg_decode_report *rep, int max, int *n, int *n_total,
                               int *n_channels)
{
    if (n) *n = 0;
    if (n_total) *n_total = 0;
    if (n_channels) *n_channels = 0;
    if (!c || !start_epoch || !n || !n_total) return CWSLG_ERR_ARG;
    if (group != CWSLG_GROUP_FT8) return fail(c, CWSLG_ERR_ARG, "decode reports exist for the FT8 group only (group %d)", group);
    return fetch_decodes_impl(c, group, start_epoch, dec, rep, max, n, n_total, n_channels, FETCH_REPORTS);
}

// The FT4 group's call (ft4soft_kernels.hpp: ft4_report_kernel; the contract is the header's, "FT4 signal reports").
int cwslg_fetch_ft4_decode_reports(cwslg_ctx *c, uint64_t *start_epoch, cwslg_decode *dec, cwslg_decode_report *rep, int max, int *n, int *n_total,
                                   int *n_channels)
{
    if (n) *n = 0;
    if (n_total) *n_total = 0;
    if (n_channels) *n_channels = 0;
    if (!c || !start_epoch || !n || !n_total) return CWSLG_ERR_ARG;
    return fetch_decodes_impl(c, CWSLG_GROUP_FT4, start_epoch, dec, rep, max, n, n_total, n_channels, FETCH_REPORTS);
}

// The a-priori words of the FT8 group (ap_kernels.hpp; the contract is the header's, cwslg_fetch_ft8_ap): cwslg_fetch_decodes' ticket, epoch rule
// and serialisation, with the a-priori decode launch in front of the harvest launches and one annotate launch behind them.
int cwslg_fetch_ft8_ap(cwslg_ctx *c, uint64_t *start_epoch, cwslg_decode *dst, int max, int *n, int *n_total, int *n_channels)
{
    if (n) *n = 0;
    if (n_total) *n_total = 0;
    if (n_channels) *n_channels = 0;
    if (!c || !start_epoch || !n || !n_total || (max > 0 && !dst)) return CWSLG_ERR_ARG;
    return fetch_decodes_impl(c, CWSLG_GROUP_FT8, start_epoch, dst, nullptr, max, n, n_total, n_channels, FETCH_AP);
}

// The a-priori words of the FT4 group (the header's "FT4 a-priori decoding"): the same path under the FT4 patterns -- a wave per (record slot,
// metric set), the harvest's FT4 modes on the staging's three-set records.
int cwslg_fetch_ft4_ap(cwslg_ctx *c, uint64_t *start_epoch, cwslg_decode *dst, int max, int *n, int *n_total, int *n_channels)
{
    if (n) *n = 0;
    if (n_total) *n_total = 0;
    if (n_channels) *n_channels = 0;
    if (!c || !start_epoch || !n || !n_total || (max > 0 && !dst)) return CWSLG_ERR_ARG;
    return fetch_decodes_impl(c, CWSLG_GROUP_FT4, start_epoch, dst, nullptr, max, n, n_total, n_channels, FETCH_AP);
}

// The channel tones of a 91-bit word under the code in force: the re-encoder of the reports on its own, host work only.
static int tones_impl(cwslg_ctx *c, const uint8_t *bits, uint8_t *tones, bool ft4)
{
    if (!c || !bits || !tones) return CWSLG_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    if (!c->sync_shared.enc_ready)
        return fail(c, CWSLG_ERR_ARG, "%s", c->sync_shared.ldpc_loaded ? "no systematic code: columns 91..173 of the loaded parity-check table are singular"
                                                                : "no parity-check table loaded (cwslg_set_ldpc_code)");
    OsdGen enc;
    std::memcpy(&enc, c->sync_shared.enc_gen, sizeof(OsdGen));
    uint32_t cw[OSD_GW];
    ldpc_encode(enc, bits, cw);
    if (ft4) ft4_tones_of(cw, tones); else ft8_tones_of(cw, tones);
    return CWSLG_OK;
}
int cwslg_ft8_tones(cwslg_ctx *c, const uint8_t *bits, uint8_t *tones) { return tones_impl(c, bits, tones, false); }
int cwslg_ft4_tones(cwslg_ctx *c, const uint8_t *bits, uint8_t *tones) { return tones_impl(c, bits, tones, true); }

// FT8 signal subtraction (the header's "FT8 signal subtraction"; ft8sub_host.inc): the report call's path with the module's two launches.
int cwslg_subtract_ft8(cwslg_ctx *c, uint64_t *start_epoch, cwslg_decode *dec, cwslg_subtract_report *sub, int max, int *n, int *n_total, int *n_channels)
{
    if (n) *n = 0;
    if (n_total) *n_total = 0;
    if (n_channels) *n_channels = 0;
    if (!c || !start_epoch || !n || !n_total) return CWSLG_ERR_ARG;
    return fetch_decodes_impl(c, CWSLG_GROUP_FT8, start_epoch, dec, nullptr, max, n, n_total, n_channels, FETCH_SUBTRACT, sub);
}

// FT4 signal subtraction (the header's "FT4 signal subtraction"): the same path for the FT4 group, on lib/cwslgpu_ft4sub.hsaco's two kernels.
int cwslg_subtract_ft4(cwslg_ctx *c, uint64_t *start_epoch, cwslg_decode *dec, cwslg_subtract_report *sub, int max, int *n, int *n_total, int *n_channels)
{
    if (n) *n = 0;
    if (n_total) *n_total = 0;
    if (n_channels) *n_channels = 0;
    if (!c || !start_epoch || !n || !n_total) return CWSLG_ERR_ARG;
    return fetch_decodes_impl(c, CWSLG_GROUP_FT4, start_epoch, dec, nullptr, max, n, n_total, n_channels, FETCH_SUBTRACT, sub);
}

// A channel's residual in the stage `st` (the FT8 group's or the FT4 group's): valid only while the block's epoch is the channel's frame epoch.
// *slot: its place in the block.  A channel of the other group is in no block of this one.  Caller holds the group's harvest[].mu and c->mu.
static int residual_slot(cwslg_ctx *c, const Ft8SubStage &st, int ch_id, size_t *slot, uint64_t *start_epoch)
{
    if (ch_id < 0 || ch_id >= (int)c->chans.size() || !c->chans[ch_id].open) return fail(c, CWSLG_ERR_ARG, "bad channel id");
    const Channel &ch = c->chans[ch_id];
    if (!ch.have_frame || !st.resid_epoch || ch.frame_t0 != st.resid_epoch) return CWSLG_ERR_NO_FRAME;
    const auto it = std::find(st.resid_chans.begin(), st.resid_chans.end(), ch_id);
    if (it == st.resid_chans.end()) return CWSLG_ERR_NO_FRAME;
    *slot = (size_t)(it - st.resid_chans.begin());
    if (start_epoch) *start_epoch = st.resid_epoch;
    return CWSLG_OK;
}

// ft4: the FT4 group's stage, lock and frame length (72576); else the FT8 group's (180000)
static int fetch_residual_impl(cwslg_ctx *c, bool ft4, int ch_id, float *dst, size_t cap, size_t *n_valid, uint64_t *start_epoch)
{
    if (n_valid) *n_valid = 0;
    if (!c || !dst) return CWSLG_ERR_ARG;
    std::lock_guard<std::mutex> serial(c->harvest[ft4 ? 1 : 0].mu);
    std::lock_guard<std::mutex> g(c->mu);
    const Ft8SubStage &st = ft4 ? c->ft4sub : c->ft8sub;
    const size_t sub_n = ft4 ? F4SUB_N : F8SUB_N;
    size_t slot = 0;
    const int rc = residual_slot(c, st, ch_id, &slot, start_epoch);
    if (rc) return rc;
    if (cap < sub_n) return fail(c, CWSLG_ERR_ARG, "destination holds %zu samples, a residual has %d", cap, (int)sub_n);
    hipSetDevice(c->device);
    // (the call that wrote the block synchronised its stream before it returned)
    HIPCHK(c, hipMemcpyAsync(dst, st.d_resid + slot * sub_n, sub_n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n_valid) *n_valid = sub_n;
    return CWSLG_OK;
}

static int residual_device_ptr_impl(cwslg_ctx *c, bool ft4, int ch_id, const float **d_f32, uint64_t *start_epoch)
{
    if (d_f32) *d_f32 = nullptr;
    if (!c || !d_f32) return CWSLG_ERR_ARG;
    std::lock_guard<std::mutex> serial(c->harvest[ft4 ? 1 : 0].mu);
    std::lock_guard<std::mutex> g(c->mu);
    const Ft8SubStage &st = ft4 ? c->ft4sub : c->ft8sub;
    size_t slot = 0;
    const int rc = residual_slot(c, st, ch_id, &slot, start_epoch);
    if (rc) return rc;
    *d_f32 = st.d_resid + slot * (size_t)(ft4 ? F4SUB_N : F8SUB_N);
    return CWSLG_OK;
}

int cwslg_fetch_ft8_residual(cwslg_ctx *c, int ch_id, float *dst, size_t cap, size_t *n_valid, uint64_t *start_epoch)
{
    return fetch_residual_impl(c, false, ch_id, dst, cap, n_valid, start_epoch);
}
int cwslg_ft8_residual_device_ptr(cwslg_ctx *c, int ch_id, const float **d_f32, uint64_t *start_epoch) { return residual_device_ptr_impl(c, false, ch_id, d_f32, start_epoch); }
int cwslg_fetch_ft4_residual(cwslg_ctx *c, int ch_id, float *dst, size_t cap, size_t *n_valid, uint64_t *start_epoch)
{
    return fetch_residual_impl(c, true, ch_id, dst, cap, n_valid, start_epoch);
}
int cwslg_ft4_residual_device_ptr(cwslg_ctx *c, int ch_id, const float **d_f32, uint64_t *start_epoch) { return residual_device_ptr_impl(c, true, ch_id, d_f32, start_epoch); }

// The same two kernels on caller-supplied frames and items: temporary device buffers, the context's stream, synchronous (cwslg_ldpc_decode's
// pattern).  The items are laid out as the harvest lays out its records (head, 10 dwords each, per-frame offsets), which is what the kernels read.
// cwslg_ft8_sub_item and cwslg_ft4_sub_item have one layout; ft4 chooses the module, the frame length and the fit record.
static_assert(sizeof(cwslg_ft4_sub_item) == sizeof(cwslg_ft8_sub_item) && offsetof(cwslg_ft4_sub_item, bits) == offsetof(cwslg_ft8_sub_item, bits)
              && offsetof(cwslg_ft4_sub_item, freq_hz) == offsetof(cwslg_ft8_sub_item, freq_hz) && offsetof(cwslg_ft4_sub_item, dt_s) == offsetof(cwslg_ft8_sub_item, dt_s),
              "one item layout");
static_assert(CWSLG_FT4_FRAME_SAMPLES == F4SUB_N && CWSLG_FT8_FRAME_SAMPLES == F8SUB_N, "the header's frame lengths");
static int subtract_flat_impl(cwslg_ctx *c, bool ft4, const float *audio, int n_frames, const cwslg_ft8_sub_item *items, int n_items, cwslg_subtract_report *sub,
                              float *residual)
{
    if (!c || n_frames < 1 || n_items < 0 || !audio || (n_items > 0 && (!items || !sub))) return CWSLG_ERR_ARG;
    const size_t sub_n = ft4 ? F4SUB_N : F8SUB_N, sub_rec_words = ft4 ? F4SUB_REC_WORDS : F8SUB_REC_WORDS;
    std::lock_guard<std::mutex> report_serial(c->report_mu);       // (the encoder's device copy, as the report calls)
    std::lock_guard<std::mutex> g(c->mu);
    std::vector<unsigned> offsets((size_t)n_frames, 0u), out((size_t)HARVEST_HEAD_WORDS + (size_t)n_items * HARVEST_REC_WORDS, 0u);
    out[0] = (unsigned)n_items;
    int frame = 0;
    for (int i = 0; i < n_items; ++i) {
        const cwslg_ft8_sub_item &it = items[i];
        if (it.frame < frame || it.frame >= n_frames) return fail(c, CWSLG_ERR_ARG, "item %d: frame %d out of range or not in ascending order", i, it.frame);
        if (!(it.freq_hz >= 0.0f && it.freq_hz <= 6000.0f) || !(it.dt_s >= -30.0f && it.dt_s <= 30.0f))
            return fail(c, CWSLG_ERR_ARG, "item %d: freq_hz outside 0..6000 or dt_s outside -30..30", i);
        while (frame < it.frame) offsets[++frame] = (unsigned)i;
        unsigned *o = out.data() + HARVEST_HEAD_WORDS + (size_t)i * HARVEST_REC_WORDS;
        o[0] = (unsigned)it.frame;
        std::memcpy(o + 2, it.bits, 12);
        std::memcpy(o + 5, &it.freq_hz, 4);
        std::memcpy(o + 6, &it.dt_s, 4);
    }
    while (frame < n_frames - 1) offsets[++frame] = (unsigned)n_items;
    hipSetDevice(c->device);
    const uint32_t *d_enc = nullptr;
    int rc = ft8sub_encoder(c, &d_enc);
    if (!rc) rc = ft4 ? ft4sub_module(c) : ft8sub_module(c);
    if (rc) return rc;
    const Ft8SubStage &st = ft4 ? c->ft4sub : c->ft8sub;
    auto pad = [](size_t v) { return (v + 255) & ~size_t(255); };
    const size_t frame_bytes = (size_t)n_frames * sub_n * sizeof(float);
    const size_t desc_at = 2 * pad(frame_bytes), off_at = desc_at + pad((size_t)n_frames * sizeof(SubDesc)), out_at = off_at + pad(offsets.size() * sizeof(unsigned));
    const size_t rep_at = out_at + pad(out.size() * sizeof(unsigned)), recs_at = rep_at + pad((size_t)n_items * F8SUB_REP_WORDS * sizeof(unsigned));
    const size_t total = recs_at + (size_t)n_items * sub_rec_words * sizeof(unsigned);
    char *d = nullptr;
    HIPCHK(c, hipMalloc((void **)&d, total));
    std::vector<SubDesc> descs((size_t)n_frames);
    for (int f = 0; f < n_frames; ++f) {
        descs[f].frame = (const float *)d + (size_t)f * sub_n;
        descs[f].resid = (float *)(d + pad(frame_bytes)) + (size_t)f * sub_n;
        descs[f].n_valid = (int)sub_n;
    }
    hipError_t e = hipMemcpyAsync(d, audio, frame_bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d + desc_at, descs.data(), descs.size() * sizeof(SubDesc), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d + off_at, offsets.data(), offsets.size() * sizeof(unsigned), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d + out_at, out.data(), out.size() * sizeof(unsigned), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
        e = ft8sub_launch(st.fit, st.apply, c->stream, (const SubDesc *)(d + desc_at), (const unsigned *)(d + off_at), (const unsigned *)(d + out_at), d_enc,
                          (unsigned *)(d + recs_at), (unsigned *)(d + rep_at), n_frames, n_items, n_items, ft4 ? F4SUB_NTILE : F8SUB_NTILE);
    if (e == hipSuccess && n_items > 0) e = hipMemcpyAsync(sub, d + rep_at, (size_t)n_items * sizeof(cwslg_subtract_report), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && residual) e = hipMemcpyAsync(residual, d + pad(frame_bytes), frame_bytes, hipMemcpyDeviceToHost, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);       // (the host vectors above live until here)
    (void)hipFree(d);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(c, CWSLG_ERR_HIP, "%s failed: %s", ft4 ? "cwslg_ft4_subtract_flat" : "cwslg_ft8_subtract_flat", hipGetErrorString(e));
    return CWSLG_OK;
}

int cwslg_ft8_subtract_flat(cwslg_ctx *c, const float *audio, int n_frames, const cwslg_ft8_sub_item *items, int n_items, cwslg_subtract_report *sub,
                            float *residual)
{
    return subtract_flat_impl(c, false, audio, n_frames, items, n_items, sub, residual);
}

int cwslg_ft4_subtract_flat(cwslg_ctx *c, const float *audio, int n_frames, const cwslg_ft4_sub_item *items, int n_items, cwslg_subtract_report *sub,
                            float *residual)
{
    return subtract_flat_impl(c, true, audio, n_frames, reinterpret_cast<const cwslg_ft8_sub_item *>(items), n_items, sub, residual);
}

int cwslg_sync_debug_fetch(cwslg_ctx *c, int ch_id, int what, void *dst, size_t cap_bytes, size_t *n_items, int *row_len)
{
    if (!c || !dst) return CWSLG_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    if (ch_id < 0 || ch_id >= (int)c->chans.size() || !c->chans[ch_id].open) return fail(c, CWSLG_ERR_ARG, "bad channel id");
    Channel &ch = c->chans[ch_id];
    if (!ch.have_frame || !ch.syncbuf.d_block) return CWSLG_ERR_NO_FRAME;
    const void *src = nullptr;
    size_t items = 0;
    switch (what) {
    case 0: src = ch.syncbuf.d_spectra; items = (size_t)(ch.syncbuf.ft4 ? FT4_NHSYM : FT8_NHSYM) * ch.syncbuf.nbins; break;
    case 1: src = ch.syncbuf.d_red; items = FT8_NH1 + 1; break;
    case 2: src = ch.syncbuf.d_red2; items = FT8_NH1 + 1; break;
    case 3: src = ch.syncbuf.d_jpeak; items = FT8_NH1 + 1; break;
    case 4: src = ch.syncbuf.d_jpeak2; items = FT8_NH1 + 1; break;
    case 5: src = ch.syncbuf.d_cx; items = 2 * (size_t)(F4C_N2 + 1); break;          // FT4 frame spectrum, complex
    case 6: src = ch.syncbuf.d_cd_dbg; items = 2 * (size_t)F4C_NP; break;             // baseband of candidate 0, complex
    default: return fail(c, CWSLG_ERR_ARG, "bad selector");
    }
    if (!src) return CWSLG_ERR_NO_FRAME;
    if (cap_bytes < items * 4) return fail(c, CWSLG_ERR_ARG, "destination too small");
    hipSetDevice(c->device);
    HIPCHK(c, hipMemcpyAsync(dst, src, items * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, sync_streams(c));
    if (n_items) *n_items = items;
    if (row_len) *row_len = ch.syncbuf.nbins;
    return CWSLG_OK;
}

} // extern "C"
