// Stand-alone host program over csrc/ldpc_host.hpp (built by tests/test_ldpc_ref.py with g++ -ffp-contract=off): evaluates T, A, the CRC-14 and the
// table validation / derivation on the inputs of a binary file and writes the results to another, for a bit-for-bit comparison with tests/ldpc_ref.py.
//   in : u32 nT, float[nT] | u32 nA, float[nA] | u32 nC, nC x (u64 lo, u64 hi) | u32 nTab, nTab x u8[581]
//   out: float[nT] | float[nA] | nC x (u32 crc, u32 field) | nTab x (i32 verdict, LdpcTables -- zeros when rejected)
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

struct Word { uint64_t lo, hi; };
struct Table { uint8_t nm[LDPC_M * LDPC_ROWMAX]; };

int main(int argc, char **argv)
{
    if (argc != 3) return 1;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 1;
    for (float x : get<float>(in)) { const float y = ldpc_T(x); fwrite(&y, 4, 1, out); }
    for (float x : get<float>(in)) { const float y = ldpc_A(x); fwrite(&y, 4, 1, out); }
    for (const Word &w : get<Word>(in)) {
        const uint32_t r[2] = {ldpc_crc14(w.lo, w.hi), ldpc_crc_field(w.lo, w.hi)};
        fwrite(r, 4, 2, out);
    }
    for (const Table &t : get<Table>(in)) {
        LdpcTables d;
        memset(&d, 0, sizeof(d));
        const int32_t verdict = ldpc_derive(t.nm, &d);
        fwrite(&verdict, 4, 1, out);
        fwrite(&d, sizeof(d), 1, out);
    }
    fclose(in);
    return fclose(out) ? 1 : 0;
}
