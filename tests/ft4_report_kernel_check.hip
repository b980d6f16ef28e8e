// ft4_report_kernel_check.hip -- test tooling: ft4_report_kernel (csrc/ft4soft_kernels.hpp) driven directly on frame
// spectra, sync records and decode records a test wrote, launched through ft4_report_launch as cwslg_fetch_ft4_decode_reports launches it, with
// the tables the library uploads (ft4c_host_tables).  tests/ft4_report_kernel_cases.py writes the case file and reads the result file;
// tests/test_gpu_ft4_report_kernel.py runs this program once for all cases.  Built with the product's flags, without -shared -fPIC.
//
//   ft4_report_kernel_check CASES RESULTS
//
// CASES (little-endian 32-bit words, then raw arrays):  "F4K1", n_cases, n_spectra, then n_spectra frame spectra (float2[36289] each); per case:
// n_chan, n_total, lim, the encoder (546 words), offsets[n_chan]; per channel: the index of its spectrum, cap, cnt, nrec[cap] and the sync
// records (Ft4Rec[cap][3], 32 bytes each); then min(n_total, lim) decode records of 40 bytes.  RESULTS: "F4R1", n_cases; per case: lim,
// rep[4 * (lim + 8)] -- filled with 0xAB before the launch, so what the kernel did not write is still 0xAB.
//
// The case file is vetted before anything is launched (offsets ascending from 0, every record's entry below the number of records its channel's
// nrec[] walk yields, nrec in 0..3, cnt and cap in range, every spectrum index valid): the kernel is never handed an index it could leave its
// blocks with.  f1_hz and ibest need no vetting -- the kernel bounds every bin and sample it reads -- but must be finite and small enough for
// int arithmetic.  Every HIP call is checked: the first error is printed and the program exits non-zero without another call into the runtime.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "demod_kernels.hpp"
#include "ft4soft_kernels.hpp"

using namespace cwslg;

static int g_case = -1;

#define CHK(call)                                                                                                                     \
    do {                                                                                                                              \
        const hipError_t e_ = (call);                                                                                                 \
        if (e_ != hipSuccess) {                                                                                                       \
            std::fprintf(stderr, "ft4_report_kernel_check: case %d: %s: %s\n", g_case, #call, hipGetErrorString(e_));                 \
            std::_Exit(3);                                                                                                            \
        }                                                                                                                             \
    } while (0)

constexpr int GUARD_RECS = 8, MAX_CHAN = 4096, MAX_OUT = 1 << 12, ENC_WORDS = REPORT_ENC_ROWS * REPORT_ENC_WORDS, MAX_SPECTRA = 16;
constexpr size_t CX_BYTES = (size_t)(F4C_N2 + 1) * sizeof(float2);

[[noreturn]] static void die(const char *what)
{
    std::fprintf(stderr, "ft4_report_kernel_check: case %d: %s\n", g_case, what);
    std::exit(2);
}

struct Reader {
    const std::vector<unsigned char> &b;
    size_t at = 0;
    const unsigned char *take(size_t n)
    {
        if (n > b.size() - at) die("the case file ends early");
        at += n;
        return b.data() + at - n;
    }
    int word()
    {
        int v;
        std::memcpy(&v, take(4), 4);
        return v;
    }
};

static size_t pad(size_t v) { return (v + 255) & ~size_t(255); }

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: ft4_report_kernel_check CASES RESULTS\n"); return 2; }
    std::vector<unsigned char> in;
    {
        FILE *f = std::fopen(argv[1], "rb");
        if (!f) die("cannot open the case file");
        unsigned char buf[1 << 16];
        size_t n;
        while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) in.insert(in.end(), buf, buf + n);
        std::fclose(f);
    }
    Reader rd{in};
    if (std::memcmp(rd.take(4), "F4K1", 4) != 0) die("not a case file");
    const int n_cases = rd.word(), n_spectra = rd.word();
    if (n_cases < 0 || n_cases > 4096 || n_spectra < 1 || n_spectra > MAX_SPECTRA) die("bad file header");
    std::vector<unsigned> result;
    unsigned magic;
    std::memcpy(&magic, "F4R1", 4);
    result.push_back(magic);
    result.push_back((unsigned)n_cases);

    hipStream_t stream;
    CHK(hipSetDevice(0));
    CHK(hipStreamCreate(&stream));
    // the tables, as the library uploads them, and the spectra the cases share
    const Ft4HostTables ht = ft4c_host_tables();
    float2 *d_t = nullptr;
    float *d_win = nullptr;
    unsigned char *d_cx = nullptr;
    CHK(hipMalloc((void **)&d_t, ht.t.size() * sizeof(float2)));
    CHK(hipMalloc((void **)&d_win, ht.win.size() * sizeof(float)));
    CHK(hipMalloc((void **)&d_cx, pad(CX_BYTES) * (size_t)n_spectra));
    CHK(hipMemcpy(d_t, ht.t.data(), ht.t.size() * sizeof(float2), hipMemcpyHostToDevice));
    CHK(hipMemcpy(d_win, ht.win.data(), ht.win.size() * sizeof(float), hipMemcpyHostToDevice));
    for (int s = 0; s < n_spectra; ++s) CHK(hipMemcpy(d_cx + pad(CX_BYTES) * (size_t)s, rd.take(CX_BYTES), CX_BYTES, hipMemcpyHostToDevice));
    const Ft4Tables tb = ht.device(d_t, d_win);

    for (g_case = 0; g_case < n_cases; ++g_case) {
        const int n_chan = rd.word(), n_total = rd.word(), lim = rd.word();
        if (n_chan < 1 || n_chan > MAX_CHAN || n_total < 0 || n_total > MAX_OUT || lim < 0 || lim > MAX_OUT) die("bad case header");
        const int n_rec = n_total < lim ? n_total : lim;
        // one block for everything of the case: descriptors | offsets | encoder | out (head + lim records) | rep (lim + guard) | per channel: cnt, nrec, records
        const size_t o_off = pad((size_t)n_chan * sizeof(Ft4ReportDesc)), o_enc = o_off + pad((size_t)n_chan * 4), o_out = o_enc + pad((size_t)ENC_WORDS * 4);
        const size_t out_words = HARVEST_HEAD_WORDS + (size_t)HARVEST_REC_WORDS * (size_t)lim, o_rep = o_out + pad(out_words * 4);
        const size_t rep_words = (size_t)REPORT_WORDS * ((size_t)lim + GUARD_RECS), o_chan = o_rep + pad(rep_words * 4);
        std::vector<unsigned char> h(o_chan);
        std::memset(h.data() + o_out, 0xAB, o_chan - o_out);
        std::memcpy(h.data() + o_enc, rd.take((size_t)ENC_WORDS * 4), (size_t)ENC_WORDS * 4);
        std::memcpy(h.data() + o_off, rd.take((size_t)n_chan * 4), (size_t)n_chan * 4);
        std::vector<unsigned> offs((size_t)n_chan);
        std::memcpy(offs.data(), h.data() + o_off, (size_t)n_chan * 4);
        if (offs[0] != 0u) die("offsets do not start at 0");
        for (int c = 1; c < n_chan; ++c) if (offs[c] < offs[c - 1]) die("offsets descend");
        struct Chan { int spectrum, cap, cnt, n_entries; size_t cnt_at, nrec, rec; };
        std::vector<Chan> chans((size_t)n_chan);
        for (Chan &c : chans) {
            c.spectrum = rd.word(); c.cap = rd.word(); c.cnt = rd.word();
            if (c.spectrum < 0 || c.spectrum >= n_spectra || c.cap < 1 || c.cap > SYNC_MAXCAND_CAP || c.cnt < 0 || c.cnt > 4 * SYNC_MAXCAND_CAP) die("bad channel header");
            auto put = [&](const void *src, size_t n) {
                const size_t o = h.size();
                h.resize(o + pad(n));
                std::memcpy(h.data() + o, src, n);
                return o;
            };
            const size_t nrec_bytes = (size_t)c.cap * 4, rec_bytes = (size_t)c.cap * 3 * sizeof(Ft4Rec);
            c.cnt_at = put(&c.cnt, 4);
            const unsigned char *nr = rd.take(nrec_bytes);
            c.nrec = put(nr, nrec_bytes);
            const unsigned char *rc = rd.take(rec_bytes);
            c.rec = put(rc, rec_bytes);
            const int n = c.cnt < c.cap ? c.cnt : c.cap;
            c.n_entries = 0;
            for (int k = 0; k < c.cap; ++k) {
                int v;
                std::memcpy(&v, nr + 4 * (size_t)k, 4);
                if (v < 0 || v > 3) die("nrec out of range");
                if (k < n) c.n_entries += v;
                for (int r = 0; r < v; ++r) {
                    Ft4Rec x;
                    std::memcpy(&x, rc + ((size_t)k * 3 + (size_t)r) * sizeof(Ft4Rec), sizeof x);
                    if (!std::isfinite(x.f1_hz) || std::fabs(x.f1_hz) > 1.0e6f || x.ibest < -(1 << 20) || x.ibest > (1 << 20)) die("a sync record out of range");
                }
            }
        }
        unsigned head[HARVEST_HEAD_WORDS] = {(unsigned)n_total, 0u, 0u, 0u};
        std::memcpy(h.data() + o_out, head, sizeof head);
        std::memcpy(h.data() + o_out + sizeof head, rd.take((size_t)n_rec * 40), (size_t)n_rec * 40);
        // vet: record p belongs to the last channel c with offsets[c] <= p; its entry is one of that channel's records
        for (int p = 0; p < n_rec; ++p) {
            int c = 0;
            while (c + 1 < n_chan && offs[c + 1] <= (unsigned)p) ++c;
            unsigned w1;
            std::memcpy(&w1, h.data() + o_out + sizeof head + (size_t)p * 40 + 4, 4);
            if ((int)(w1 & 0xffffu) >= chans[(size_t)c].n_entries) die("a record's entry lies beyond its channel's records");
        }
        unsigned char *d = nullptr;
        CHK(hipMalloc((void **)&d, h.size()));
        for (int i = 0; i < n_chan; ++i) {
            const Chan &c = chans[(size_t)i];
            Ft4ReportDesc r{};
            r.cx = (const float2 *)(d_cx + pad(CX_BYTES) * (size_t)c.spectrum);
            r.rec = (const Ft4Rec *)(d + c.rec);
            r.nrec = (const int *)(d + c.nrec);
            r.cnt = (const int *)(d + c.cnt_at);
            r.cap = c.cap;
            std::memcpy(h.data() + (size_t)i * sizeof(Ft4ReportDesc), &r, sizeof r);
        }
        CHK(hipMemcpyAsync(d, h.data(), h.size(), hipMemcpyHostToDevice, stream));
        ft4_report_launch(stream, (const Ft4ReportDesc *)d, (const unsigned *)(d + o_off), (const unsigned *)(d + o_out), (const uint32_t *)(d + o_enc),
                          (unsigned *)(d + o_rep), tb, d_t + ht.o32, n_chan, lim);
        CHK(hipGetLastError());
        const size_t r0 = result.size();
        result.resize(r0 + 1 + rep_words);
        result[r0] = (unsigned)lim;
        CHK(hipMemcpyAsync(&result[r0 + 1], d + o_rep, rep_words * 4, hipMemcpyDeviceToHost, stream));
        CHK(hipStreamSynchronize(stream));
        CHK(hipFree(d));
    }
    CHK(hipFree(d_cx));
    CHK(hipFree(d_win));
    CHK(hipFree(d_t));
    CHK(hipStreamDestroy(stream));
    g_case = -1;
    if (rd.at != in.size()) die("bytes left over in the case file");
    FILE *f = std::fopen(argv[2], "wb");
    if (!f) die("cannot open the result file");
    const bool ok = std::fwrite(result.data(), 4, result.size(), f) == result.size();
    if (std::fclose(f) != 0 || !ok) die("cannot write the result file");
    std::printf("ft4_report_kernel_check: %d cases\n", n_cases);
    return 0;
}
