// Stand-alone host program over csrc/ldpc_host.hpp (built by tests/test_osd_ref.py with g++ -ffp-contract=off, and once more with
// -fsanitize=address,undefined): derives rank and generator of parity-check tables and runs the host OSD (osd_host) on sets of metrics, for a
// bit-for-bit comparison with tests/osd_ref.py.
//   in : u32 nTab, nTab x u8[581] | u32 nSet, nSet x (i32 table, i32 order, float[174])
//   out: nTab x (i32 verdict, i32 rank, OsdGen -- zeros unless verdict 0 and rank 83) | nSet x cwslg_osd_msg (24 bytes; zeros when the set's
//        table has no generator)
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
struct Set { int32_t table, order; float llr[LDPC_N]; };

int main(int argc, char **argv)
{
    if (argc != 3) return 1;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 1;
    std::vector<OsdGen> gens;
    std::vector<bool> ok;
    for (const Table &t : get<Table>(in)) {
        LdpcTables d;
        OsdGen g;
        memset(&g, 0, sizeof(g));
        int32_t head[2] = {ldpc_derive(t.nm, &d), -1};
        if (head[0] == 0) head[1] = ldpc_generator(d, &g);
        fwrite(head, 4, 2, out);
        fwrite(&g, sizeof(g), 1, out);
        gens.push_back(g);
        ok.push_back(head[0] == 0 && head[1] == LDPC_M);
    }
    for (const Set &s : get<Set>(in)) {
        OsdRec r;
        memset(&r, 0, sizeof(r));
        if (s.table >= 0 && s.table < (int)gens.size() && ok[s.table] && s.order >= 0 && s.order <= 2) osd_host(gens[s.table], s.llr, s.order, &r);
        fwrite(&r, sizeof(r), 1, out);
    }
    fclose(in);
    return fclose(out) ? 1 : 0;
}
