// ft8sub_host.inc -- host side of the FT8 and FT4 subtractors (included by cwsl_gpu.hip in front of sync_host.inc, whose fetch_decodes_impl runs the chain call and
// whose tail holds the exported functions).  The two kernels are NOT in this library: they live in lib/cwslgpu_ft8sub.hsaco beside it
// (modules/ft8sub.hip; DESIGN.md 4.15), loaded with hipModuleLoad by the first call that subtracts and launched with hipModuleLaunchKernel.
// The FT4 subtractor is the same machinery on a code object of its own, lib/cwslgpu_ft4sub.hsaco (modules/ft4sub.hip; DESIGN.md 4.16): one loader
// and one launcher serve both, told apart by the stage, the file, the kernel names and the geometry.

namespace {

static_assert(F8SUB_DEC_HEAD_WORDS == HARVEST_HEAD_WORDS && F8SUB_DEC_WORDS == HARVEST_REC_WORDS, "the module reads the harvest's block");
static_assert(F8SUB_ENC_ROWS == REPORT_ENC_ROWS && F8SUB_ENC_WORDS == REPORT_ENC_WORDS, "the module reads the report's encoder");

static_assert(F4SUB_REP_WORDS == F8SUB_REP_WORDS, "one report record for both modes");
static_assert(F4SUB_NT == F8SUB_NT, "one launcher for both modes");

// A subtractor's module, loaded once per context into `st` from the directory this library was loaded from: the file's name, what to call it in
// an error text and its two kernels.  Caller holds c->mu and has set the device.
int sub_module(cwslg_ctx *c, Ft8SubStage &st, const char *file, const char *what, const char *fit_name, const char *apply_name)
{
    if (st.fit && st.apply) return CWSLG_OK;
    Dl_info info{};
    if (!dladdr((const void *)&cwslg_abi_version, &info) || !info.dli_fname) return fail(c, CWSLG_ERR_ARG, "cannot tell where this library was loaded from (dladdr)");
    std::string path(info.dli_fname);
    const size_t slash = path.rfind('/');
    path = (slash == std::string::npos ? std::string(".") : path.substr(0, slash)) + "/" + file;
    if (FILE *fh = std::fopen(path.c_str(), "rb")) std::fclose(fh);
    else return fail(c, CWSLG_ERR_ARG, "the %s subtractor's code object is missing: %s", what, path.c_str());
    if (!st.module) HIPCHK(c, hipModuleLoad(&st.module, path.c_str()));
    HIPCHK(c, hipModuleGetFunction(&st.fit, st.module, fit_name));
    HIPCHK(c, hipModuleGetFunction(&st.apply, st.module, apply_name));
    return CWSLG_OK;
}
int ft8sub_module(cwslg_ctx *c) { return sub_module(c, c->ft8sub, "cwslgpu_ft8sub.hsaco", "FT8", "ft8_sub_fit_kernel", "ft8_sub_apply_kernel"); }
int ft4sub_module(cwslg_ctx *c) { return sub_module(c, c->ft4sub, "cwslgpu_ft4sub.hsaco", "FT4", "ft4_sub_fit_kernel", "ft4_sub_apply_kernel"); }

// The encoder's device copy, as the report calls keep it.  Caller holds report_mu and c->mu.
int ft8sub_encoder(cwslg_ctx *c, const uint32_t **d_enc)
{
    SyncShared &s = c->sync_shared;
    if (!s.enc_ready)
        return fail(c, CWSLG_ERR_ARG, "%s", s.ldpc_loaded ? "signal subtraction needs a systematic code: columns 91..173 of the loaded parity-check table are singular"
                                                          : "signal subtraction needs a parity-check table (cwslg_set_ldpc_code)");
    if (!s.d_encgen) HIPCHK(c, hipMalloc(&s.d_encgen, sizeof(OsdGen)));
    if (s.enc_dirty) {
        HIPCHK(c, hipMemcpy(s.d_encgen, s.enc_gen, sizeof(OsdGen), hipMemcpyHostToDevice));
        s.enc_dirty = false;
    }
    *d_enc = (const uint32_t *)s.d_encgen;
    return CWSLG_OK;
}

// Both launches on stream `s`: the fit over the n_emit emitted records (none: no launch), then the apply over every channel and each of the
// frame's n_tile time tiles (F8SUB_NTILE, F4SUB_NTILE).
hipError_t ft8sub_launch(hipFunction_t fit, hipFunction_t apply, hipStream_t s, const SubDesc *d_desc, const unsigned *d_offsets, const unsigned *d_out,
                         const uint32_t *d_enc, unsigned *d_recs, unsigned *d_rep, int n_chan, int n_emit, int lim, int n_tile = F8SUB_NTILE)
{
    hipError_t e = hipSuccess;
    if (n_emit > 0) {
        void *args[] = {&d_desc, &d_offsets, &d_out, &d_enc, &d_recs, &d_rep, &n_chan, &lim};
        e = hipModuleLaunchKernel(fit, (unsigned)n_emit, 1, 1, F8SUB_NT, 1, 1, 0, s, args, nullptr);
        if (e != hipSuccess) return e;
    }
    const unsigned *c_recs = d_recs;
    void *args[] = {&d_desc, &d_offsets, &d_out, &c_recs, &n_chan, &lim};
    return hipModuleLaunchKernel(apply, (unsigned)n_tile, (unsigned)n_chan, 1, F8SUB_NT, 1, 1, 0, s, args, nullptr);
}

} // namespace
