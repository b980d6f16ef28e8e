// Stand-alone host program over csrc/ldpc_host.hpp (built by tests/test_ft4_decode_reports_ref.py with g++ -ffp-contract=off, and once more with
// -fsanitize=address,undefined): the systematic encoder of parity-check tables (ldpc_encoder) and the 103 FT4 tones of 91-bit words
// (ldpc_encode, ft4_tones_of), for a bit-for-bit comparison with tests/ft4_decode_reports_ref.py and tests/ldpc_cases.py.
//   in : u32 nTab, nTab x u8[581] | u32 nWord, nWord x (i32 table, u8[12] bits)
//   out: nTab x (i32 verdict of ldpc_derive, i32 systematic) | nWord x (u32 cw[6], u8 tones[103], u8 0 -- all zeros when the word's table has
//        no encoder: a table with singular parity columns is refused)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../cwsl_digi_amd/csrc/ldpc_host.hpp"

using namespace cwslg;

template <class T> static std::vector<T> get(FILE *f)
{
    uint32_t n = 0;
    if (fread(&n, 4, 1, f) != 1) exit(2);
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) exit(2);
    return v;
}

struct Table { uint8_t nm[LDPC_M * LDPC_ROWMAX]; };
struct Word { int32_t table; uint8_t bits[12]; };

int main(int argc, char **argv)
{
    if (argc != 3) return 1;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 1;
    std::vector<OsdGen> encs;
    std::vector<bool> ok;
    for (const Table &t : get<Table>(in)) {
        LdpcTables d;
        OsdGen g;
        memset(&g, 0, sizeof(g));
        int32_t head[2] = {ldpc_derive(t.nm, &d), 0};
        if (head[0] == 0) head[1] = ldpc_encoder(d, &g) ? 1 : 0;
        fwrite(head, 4, 2, out);
        encs.push_back(g);
        ok.push_back(head[0] == 0 && head[1] == 1);
    }
    for (const Word &w : get<Word>(in)) {
        uint32_t cw[OSD_GW] = {0};
        uint8_t tones[104] = {0};
        if (w.table >= 0 && w.table < (int)encs.size() && ok[w.table]) {
            ldpc_encode(encs[w.table], w.bits, cw);
            ft4_tones_of(cw, tones);
        }
        fwrite(cw, 4, OSD_GW, out);
        fwrite(tones, 1, 104, out);
    }
    fclose(in);
    return fclose(out) ? 1 : 0;
}
