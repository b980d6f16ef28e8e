// ft8sub_host.inc -- host side of the FT8 subtractor (included by cwsl_gpu.hip in front of sync_host.inc, whose fetch_decodes_impl runs the chain call and
// whose tail holds the exported functions).  The two kernels are NOT in this library: they live in lib/cwslgpu_ft8sub.hsaco beside it
// (modules/ft8sub.hip; DESIGN.md 4.15), loaded with hipModuleLoad by the first call that subtracts and launched with hipModuleLaunchKernel.

namespace {

static_assert(F8SUB_DEC_HEAD_WORDS == HARVEST_HEAD_WORDS && F8SUB_DEC_WORDS == HARVEST_REC_WORDS, "the module reads the harvest's block");
static_assert(F8SUB_ENC_ROWS == REPORT_ENC_ROWS && F8SUB_ENC_WORDS == REPORT_ENC_WORDS, "the module reads the report's encoder");

// The module, loaded once per context from the directory this library was loaded from.  Caller holds c->mu and has set the device.
int ft8sub_module(cwslg_ctx *c)
{
    Ft8SubStage &st = c->ft8sub;
    if (st.fit && st.apply) return CWSLG_OK;
    Dl_info info{};
    if (!dladdr((const void *)&cwslg_abi_version, &info) || !info.dli_fname) return fail(c, CWSLG_ERR_ARG, "cannot tell where this library was loaded from (dladdr)");
    std::string path(info.dli_fname);
    const size_t slash = path.rfind('/');
    path = (slash == std::string::npos ? std::string(".") : path.substr(0, slash)) + "/cwslgpu_ft8sub.hsaco";
    if (FILE *fh = std::fopen(path.c_str(), "rb")) std::fclose(fh);
    else return fail(c, CWSLG_ERR_ARG, "the FT8 subtractor's code object is missing: %s", path.c_str());
    if (!st.module) HIPCHK(c, hipModuleLoad(&st.module, path.c_str()));
    HIPCHK(c, hipModuleGetFunction(&st.fit, st.module, "ft8_sub_fit_kernel"));
    HIPCHK(c, hipModuleGetFunction(&st.apply, st.module, "ft8_sub_apply_kernel"));
    return CWSLG_OK;
}

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

// Both launches on stream `s`: the fit over the n_emit emitted records (none: no launch), then the apply over every channel.
hipError_t ft8sub_launch(hipFunction_t fit, hipFunction_t apply, hipStream_t s, const SubDesc *d_desc, const unsigned *d_offsets, const unsigned *d_out,
                         const uint32_t *d_enc, unsigned *d_recs, unsigned *d_rep, int n_chan, int n_emit, int lim)
{
    hipError_t e = hipSuccess;
    if (n_emit > 0) {
        void *args[] = {&d_desc, &d_offsets, &d_out, &d_enc, &d_recs, &d_rep, &n_chan, &lim};
        e = hipModuleLaunchKernel(fit, (unsigned)n_emit, 1, 1, F8SUB_NT, 1, 1, 0, s, args, nullptr);
        if (e != hipSuccess) return e;
    }
    const unsigned *c_recs = d_recs;
    void *args[] = {&d_desc, &d_offsets, &d_out, &c_recs, &n_chan, &lim};
    return hipModuleLaunchKernel(apply, F8SUB_NTILE, (unsigned)n_chan, 1, F8SUB_NT, 1, 1, 0, s, args, nullptr);
}

} // namespace
