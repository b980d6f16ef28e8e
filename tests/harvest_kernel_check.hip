// harvest_kernel_check.hip -- test tooling: decode_harvest_kernel (csrc/harvest_kernels.hpp) driven directly on records a test wrote, launched
// through harvest_launch as cwslg_fetch_decodes launches it.  tests/harvest_kernel_cases.py writes the case file and reads the result file;
// tests/test_gpu_harvest_kernel.py runs this program once for all cases.  Built with the product's flags, without -shared -fPIC.
//
//   harvest_kernel_check CASES RESULTS
//
// CASES (little-endian 32-bit words, then raw record arrays):  "HVK1", n_cases; per case: ft4, max_out, n_chan; per channel: ch_id, cap, cnt,
// osd_null, then the list (FT8: Cand[cap], 20 bytes each; FT4: Ft4Rec[cap][3], 32 bytes each), FT4 only nrec[cap], the decode records (FT8: 20
// bytes x cap; FT4: 60 bytes x cap x 3) and the OSD records (FT8: 24 bytes x cap; FT4: 72 bytes x cap x 3).
// RESULTS: "HVR1", n_cases; per case: n_chan, max_out, counts[n_chan + 8], offsets[n_chan + 8], out[4 + 10 * (max_out + 8)] -- each block filled
// with 0xAB before the launches, so what the kernel did not write is still 0xAB.
//
// Every HIP call is checked: the first error is printed and the program exits non-zero without another call into the runtime.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "demod_kernels.hpp"
#include "harvest_kernels.hpp"

using namespace cwslg;

#define CHK(call)                                                                                                                     \
    do {                                                                                                                              \
        const hipError_t e_ = (call);                                                                                                 \
        if (e_ != hipSuccess) {                                                                                                       \
            std::fprintf(stderr, "harvest_kernel_check: case %d: %s: %s\n", g_case, #call, hipGetErrorString(e_));                    \
            std::_Exit(3);                                                                                                            \
        }                                                                                                                             \
    } while (0)

static int g_case = -1;
constexpr int GUARD_RECS = 8, GUARD_WORDS = 8, MAX_CHAN = 4096, MAX_OUT = 1 << 20;
constexpr size_t LIST_BYTES[2] = {20, 3 * 32}, MSG_BYTES[2] = {20, 3 * 60}, OSD_BYTES[2] = {24, 3 * 72};      // per list entry / candidate

[[noreturn]] static void die(const char *what)
{
    std::fprintf(stderr, "harvest_kernel_check: case %d: %s\n", g_case, what);
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
    if (argc != 3) { std::fprintf(stderr, "usage: harvest_kernel_check CASES RESULTS\n"); return 2; }
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
    if (std::memcmp(rd.take(4), "HVK1", 4) != 0) die("not a case file");
    const int n_cases = rd.word();
    if (n_cases < 0 || n_cases > 4096) die("bad case count");
    std::vector<unsigned> result;
    unsigned magic;
    std::memcpy(&magic, "HVR1", 4);
    result.push_back(magic);
    result.push_back((unsigned)n_cases);

    hipStream_t stream;
    CHK(hipSetDevice(0));
    CHK(hipStreamCreate(&stream));
    for (g_case = 0; g_case < n_cases; ++g_case) {
        const int ft4 = rd.word(), max_out = rd.word(), n_chan = rd.word();
        if ((ft4 != 0 && ft4 != 1) || max_out < 0 || max_out > MAX_OUT || n_chan < 1 || n_chan > MAX_CHAN) die("bad case header");
        // one block for everything of the case: descriptors | counts | offsets | out | per channel: cnt, list, nrec, msg, osd
        const size_t desc_bytes = pad((size_t)n_chan * sizeof(HarvestDesc)), cnt_words = (size_t)n_chan + GUARD_WORDS, cnt_bytes = pad(cnt_words * 4);
        const size_t out_words = HARVEST_HEAD_WORDS + (size_t)HARVEST_REC_WORDS * ((size_t)max_out + GUARD_RECS), out_bytes = pad(out_words * 4);
        const size_t o_counts = desc_bytes, o_offsets = o_counts + cnt_bytes, o_out = o_offsets + cnt_bytes, o_chan = o_out + out_bytes;
        std::vector<unsigned char> h(o_chan);
        std::memset(h.data() + o_counts, 0xAB, o_chan - o_counts);
        struct Chan { int ch_id, cap, osd_null; size_t cnt, list, nrec, msg, osd; };
        std::vector<Chan> chans((size_t)n_chan);
        for (Chan &c : chans) {
            c.ch_id = rd.word(); c.cap = rd.word();
            const int cnt = rd.word();
            c.osd_null = rd.word();
            if (c.cap < 1 || c.cap > SYNC_MAXCAND_CAP || (c.osd_null != 0 && c.osd_null != 1)) die("bad channel header");     // the arrays hold cap entries: the kernel reads none beyond min(cnt, cap, 600)
            auto put = [&](const void *src, size_t n) {
                const size_t o = h.size();
                h.resize(o + pad(n));
                std::memcpy(h.data() + o, src, n);
                return o;
            };
            c.cnt = put(&cnt, 4);
            const size_t cap = (size_t)c.cap;
            c.list = put(rd.take(cap * LIST_BYTES[ft4]), cap * LIST_BYTES[ft4]);
            c.nrec = ft4 ? put(rd.take(cap * 4), cap * 4) : 0;
            c.msg = put(rd.take(cap * MSG_BYTES[ft4]), cap * MSG_BYTES[ft4]);
            c.osd = put(rd.take(cap * OSD_BYTES[ft4]), cap * OSD_BYTES[ft4]);
        }
        unsigned char *d = nullptr;
        CHK(hipMalloc((void **)&d, h.size()));
        for (int i = 0; i < n_chan; ++i) {
            const Chan &c = chans[(size_t)i];
            HarvestDesc hd{};
            hd.cnt = (const int *)(d + c.cnt);
            hd.list = d + c.list;
            hd.nrec = ft4 ? (const int *)(d + c.nrec) : nullptr;
            hd.msg = d + c.msg;
            hd.osd = c.osd_null ? nullptr : d + c.osd;
            hd.cap = c.cap;
            hd.ch_id = c.ch_id;
            std::memcpy(h.data() + (size_t)i * sizeof(HarvestDesc), &hd, sizeof hd);
        }
        CHK(hipMemcpyAsync(d, h.data(), h.size(), hipMemcpyHostToDevice, stream));
        harvest_launch(stream, (const HarvestDesc *)d, (unsigned *)(d + o_counts), (unsigned *)(d + o_offsets), (unsigned *)(d + o_out), n_chan, max_out, ft4);
        CHK(hipGetLastError());
        const size_t r0 = result.size();
        result.resize(r0 + 2 + 2 * cnt_words + out_words);
        result[r0] = (unsigned)n_chan;
        result[r0 + 1] = (unsigned)max_out;
        CHK(hipMemcpyAsync(&result[r0 + 2], d + o_counts, cnt_words * 4, hipMemcpyDeviceToHost, stream));
        CHK(hipMemcpyAsync(&result[r0 + 2 + cnt_words], d + o_offsets, cnt_words * 4, hipMemcpyDeviceToHost, stream));
        CHK(hipMemcpyAsync(&result[r0 + 2 + 2 * cnt_words], d + o_out, out_words * 4, hipMemcpyDeviceToHost, stream));
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
    std::printf("harvest_kernel_check: %d cases\n", n_cases);
    return 0;
}
