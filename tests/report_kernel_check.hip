// report_kernel_check.hip -- test tooling: decode_report_kernel (csrc/harvest_kernels.hpp) driven directly on planes,
// lists and decode records a test wrote, launched through report_launch as cwslg_fetch_decode_reports launches it.  tests/report_kernel_cases.py
// writes the case file and reads the result file; tests/test_gpu_report_kernel.py runs this program once for all cases.  Built with the
// product's flags, without -shared -fPIC.
//
//   report_kernel_check CASES RESULTS
//
// CASES (little-endian 32-bit words, then raw arrays):  "RPK1", n_cases; per case: n_chan, n_total, lim, the encoder (546 words), offsets[n_chan];
// per channel: nbins, cap, the plane (float[372][nbins]) and the list (Cand[cap], 20 bytes each); then min(n_total, lim) decode records of 40
// bytes.  RESULTS: "RPR1", n_cases; per case: lim, rep[4 * (lim + 8)] -- filled with 0xAB before the launch, so what the kernel did not write is
// still 0xAB.
//
// The case file is vetted before anything is launched (offsets ascending from 0, every record's entry inside its channel's list, grid positions
// in a sane range): the kernel is never handed an index it could leave its blocks with.  Every HIP call is checked: the first error is printed
// and the program exits non-zero without another call into the runtime.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "demod_kernels.hpp"
#include "harvest_kernels.hpp"

using namespace cwslg;

static int g_case = -1;

#define CHK(call)                                                                                                                     \
    do {                                                                                                                              \
        const hipError_t e_ = (call);                                                                                                 \
        if (e_ != hipSuccess) {                                                                                                       \
            std::fprintf(stderr, "report_kernel_check: case %d: %s: %s\n", g_case, #call, hipGetErrorString(e_));                     \
            std::_Exit(3);                                                                                                            \
        }                                                                                                                             \
    } while (0)

constexpr int GUARD_RECS = 8, MAX_CHAN = 4096, MAX_OUT = 1 << 16, ENC_WORDS = REPORT_ENC_ROWS * REPORT_ENC_WORDS, MAX_NBINS = 2048;

[[noreturn]] static void die(const char *what)
{
    std::fprintf(stderr, "report_kernel_check: case %d: %s\n", g_case, what);
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
    if (argc != 3) { std::fprintf(stderr, "usage: report_kernel_check CASES RESULTS\n"); return 2; }
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
    if (std::memcmp(rd.take(4), "RPK1", 4) != 0) die("not a case file");
    const int n_cases = rd.word();
    if (n_cases < 0 || n_cases > 4096) die("bad case count");
    std::vector<unsigned> result;
    unsigned magic;
    std::memcpy(&magic, "RPR1", 4);
    result.push_back(magic);
    result.push_back((unsigned)n_cases);

    hipStream_t stream;
    CHK(hipSetDevice(0));
    CHK(hipStreamCreate(&stream));
    for (g_case = 0; g_case < n_cases; ++g_case) {
        const int n_chan = rd.word(), n_total = rd.word(), lim = rd.word();
        if (n_chan < 1 || n_chan > MAX_CHAN || n_total < 0 || n_total > MAX_OUT || lim < 0 || lim > MAX_OUT) die("bad case header");
        const int n_rec = n_total < lim ? n_total : lim;
        // one block for everything of the case: descriptors | offsets | encoder | out (head + lim records) | rep (lim + guard) | per channel: plane, list
        const size_t o_off = pad((size_t)n_chan * sizeof(ReportDesc)), o_enc = o_off + pad((size_t)n_chan * 4), o_out = o_enc + pad((size_t)ENC_WORDS * 4);
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
        struct Chan { int nbins, cap; size_t plane, list; };
        std::vector<Chan> chans((size_t)n_chan);
        for (Chan &c : chans) {
            c.nbins = rd.word(); c.cap = rd.word();
            if (c.nbins < 1 || c.nbins > MAX_NBINS || c.cap < 1 || c.cap > SYNC_MAXCAND_CAP) die("bad channel header");
            auto put = [&](const void *src, size_t n) {
                const size_t o = h.size();
                h.resize(o + pad(n));
                std::memcpy(h.data() + o, src, n);
                return o;
            };
            const size_t plane_bytes = (size_t)FT8_NHSYM * (size_t)c.nbins * 4, list_bytes = (size_t)c.cap * 20;
            c.plane = put(rd.take(plane_bytes), plane_bytes);
            c.list = put(rd.take(list_bytes), list_bytes);
        }
        unsigned head[HARVEST_HEAD_WORDS] = {(unsigned)n_total, 0u, 0u, 0u};
        std::memcpy(h.data() + o_out, head, sizeof head);
        std::memcpy(h.data() + o_out + sizeof head, rd.take((size_t)n_rec * 40), (size_t)n_rec * 40);
        // vet: record p belongs to the last channel c with offsets[c] <= p; its entry lies inside that channel's list, whose positions are sane
        for (int p = 0; p < n_rec; ++p) {
            int c = 0;
            while (c + 1 < n_chan && offs[c + 1] <= (unsigned)p) ++c;
            unsigned w1;
            std::memcpy(&w1, h.data() + o_out + sizeof head + (size_t)p * 40 + 4, 4);
            const int entry = (int)(w1 & 0xffffu);
            if (entry >= chans[(size_t)c].cap) die("a record's entry lies beyond its channel's list");
            int ij[2];
            std::memcpy(ij, h.data() + chans[(size_t)c].list + (size_t)entry * 20, 8);
            if (ij[0] < 0 || ij[0] > 4096 || ij[1] < -1024 || ij[1] > 1024) die("a grid position out of range");
        }
        unsigned char *d = nullptr;
        CHK(hipMalloc((void **)&d, h.size()));
        for (int i = 0; i < n_chan; ++i) {
            ReportDesc r{};
            r.spectra = (const float *)(d + chans[(size_t)i].plane);
            r.list = d + chans[(size_t)i].list;
            r.nbins = chans[(size_t)i].nbins;
            std::memcpy(h.data() + (size_t)i * sizeof(ReportDesc), &r, sizeof r);
        }
        CHK(hipMemcpyAsync(d, h.data(), h.size(), hipMemcpyHostToDevice, stream));
        report_launch(stream, (const ReportDesc *)d, (const unsigned *)(d + o_off), (const unsigned *)(d + o_out), (const uint32_t *)(d + o_enc),
                      (unsigned *)(d + o_rep), n_chan, lim);
        CHK(hipGetLastError());
        const size_t r0 = result.size();
        result.resize(r0 + 1 + rep_words);
        result[r0] = (unsigned)lim;
        CHK(hipMemcpyAsync(&result[r0 + 1], d + o_rep, rep_words * 4, hipMemcpyDeviceToHost, stream));
        CHK(hipStreamSynchronize(stream));
        CHK(hipFree(d));
    }
    CHK(hipStreamDestroy(stream));
    g_case = -1;
    if (rd.at != in.size()) die("bytes left over in the case file");
    FILE *f = std::fopen(argv[2], "wb");
    if (!f) die("cannot open the result file");
    const bool ok = std::fwrite(result.data(), 4, result.size(), f) == result.size();
    if (std::fclose(f) != 0 || !ok) die("cannot write the result file");
    std::printf("report_kernel_check: %d cases\n", n_cases);
    return 0;
}
