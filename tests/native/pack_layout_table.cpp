// Packs test matrices with the maps and values of mvsdf_amd/csrc/pack_layout.h alone (host C++ only) for tests/test_pack_layout_host.py, which holds the
// bytes to tests/pack_ref.py:
//   pack_layout_table sizes N K [N K ...]   one text line per shape: N K mv_packed_floats mv_packed_bf16_elems
//   pack_layout_table packs N K [N K ...]   per shape, binary on stdout: the fp32 pack, the rounded fp32 pack, the one-term bf16 pack and the three-term pack
//                                           of W [N][K], then the three-term pack of W^T; W[o][k] has the bit pattern 0x3f800005 + 8 (1024 o + k)
//   pack_layout_table terms HEX [HEX ...]   one text line per float32 bit pattern: the three terms of mv_x3_term, hex
// Every map is also run backwards (mv_frag_*_at, mv_block_index): a mismatch ends the program with status 2.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "pack_layout.h"

static float element(int o, int k) {
    const uint32_t u = 0x3f800005u + 8u * (1024u * (uint32_t)o + (uint32_t)k);
    float f;
    memcpy(&f, &u, 4);
    return f;
}
// element (o, k) of the No x Ko matrix being packed (tr: W^T of W [Ko][No]), +0 outside it
static float source(int o, int k, int No, int Ko, bool tr) { return (o < No && k < Ko) ? (tr ? element(k, o) : element(o, k)) : 0.0f; }

static void must(bool ok, const char* what) {
    if (!ok) { fprintf(stderr, "pack_layout_table: %s does not invert\n", what); exit(2); }
}

enum Value { PLAIN, ROUNDED, BF16, X3 };

template <class T>
static void pack(int No, int Ko, bool tr, Value value) {
    const bool f32 = sizeof(T) == 4;
    const int terms = value == X3 ? 3 : 1, KB = f32 ? mv_kpad(Ko) / 16 : mv_bf_kb(Ko), KW = f32 ? 16 : 32, per_block = 16 * KW;
    const size_t total = terms * (f32 ? mv_packed_floats(No, Ko) : mv_packed_bf16_elems(No, Ko));
    std::vector<T> out(total);
    for (size_t idx = 0; idx < total; ++idx) {
        const int e = (int)(idx % per_block);
        const MvBlock b = mv_block_at(idx / per_block, KB, terms);
        const MvFrag f = f32 ? mv_frag_f32(e) : mv_frag_bf16(e);
        must((f32 ? mv_frag_f32_at(f.row, f.k) : mv_frag_bf16_at(f.row, f.k)) == e, "the fragment map");
        must(mv_block_index(b.ct, b.kb, KB, b.term, terms) == idx / per_block, "the block order");
        const float w = source(16 * b.ct + f.row, KW * b.kb + f.k, No, Ko, tr);
        T v;
        if (value == PLAIN || value == ROUNDED) { const float x = value == PLAIN ? w : mv_bf_round(w); memcpy(&v, &x, sizeof(T)); }
        else v = (T)(value == BF16 ? mv_f2bf(w) : mv_x3_term(w, b.term));
        out[idx] = v;
    }
    fwrite(out.data(), sizeof(T), total, stdout);
}

int main(int argc, char** argv) {
    if (argc < 3) return 1;
    if (!strcmp(argv[1], "terms")) {
        for (int i = 2; i < argc; ++i) {
            const uint32_t u = (uint32_t)strtoul(argv[i], nullptr, 16);
            float w;
            memcpy(&w, &u, 4);
            printf("%08x %04x %04x %04x\n", u, mv_x3_term(w, 0), mv_x3_term(w, 1), mv_x3_term(w, 2));
        }
        return 0;
    }
    const bool sizes = !strcmp(argv[1], "sizes");
    if (!sizes && strcmp(argv[1], "packs")) return 1;
    for (int i = 2; i + 1 < argc; i += 2) {
        const int N = atoi(argv[i]), K = atoi(argv[i + 1]);
        if (sizes) { printf("%d %d %zu %zu\n", N, K, mv_packed_floats(N, K), mv_packed_bf16_elems(N, K)); continue; }
        pack<float>(N, K, false, PLAIN);
        pack<float>(N, K, false, ROUNDED);
        pack<uint16_t>(N, K, false, BF16);
        pack<uint16_t>(N, K, false, X3);
        pack<uint16_t>(K, N, true, X3);
    }
    return 0;
}
