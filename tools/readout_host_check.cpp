// readout_host_check.cpp -- the per-thread functions of the round read-out (freddie_amd/csrc/clu_readout.h, what k_readout_exons /
// k_readout_corr of freddie_cluster.hip call) run on the host: the exon words of a problem as a lane per word computes them, their bytes
// and e, then every (member, word) lane's characters, stored as the kernel stores them -- 16 bytes at once where ro_store_halves allows,
// alone elsewhere -- into one buffer in which the members' rows start at the byte offset the input names.
// tools/readout_host_check.py feeds it problems and compares what it prints with the numpy mirror (cluster_prep.readout_words).
// Build:  g++ -O1 -g -std=c++17 -fsanitize=address,undefined -I freddie_amd/csrc tools/readout_host_check.cpp -o readout_host_check
// (every array is a std::vector read and written through at(): an index outside one stops the run)
//
// Input, whitespace separated, one problem after the other until the end of the input:
//   M R n_members row_offset | members | I rows (R x W words) | C rows (R x W) | label rows (R x LW) | informative words (W)
// Output per problem: the exon words in hex | the exon bytes | e | a line per member: its characters | "wide" and "bytes" store counts
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "clu_readout.h"

namespace {

bool read_int(long long &v) { return scanf("%lld", &v) == 1; }

long long need_int() {
    long long v;
    if (!read_int(v)) { fprintf(stderr, "input ends inside a problem\n"); exit(2); }
    return v;
}

void need_words(std::vector<unsigned> &v, size_t n) {
    v.resize(n);
    for (auto &x : v) x = (unsigned)need_int();
}

void store4(std::vector<unsigned char> &buf, size_t at, unsigned v) {
    for (int b = 0; b < 4; ++b) buf.at(at + (size_t)b) = (unsigned char)(v >> (8 * b));
}

void run_problem(int M) {
    const int R = (int)need_int(), n_mem = (int)need_int();
    const ro_i64 row_offset = need_int();
    const int W = M + 31 >= 64 ? (M + 31) / 32 : 1, LW = M + 15 >= 32 ? (M + 15) / 16 : 1;
    std::vector<int> members((size_t)n_mem);
    for (auto &c : members) c = (int)need_int();
    std::vector<unsigned> I, C, L, inf;
    need_words(I, (size_t)R * W); need_words(C, (size_t)R * W); need_words(L, (size_t)R * LW); need_words(inf, (size_t)W);
    // ---- k_readout_exons: a lane per word, a loop over the members
    std::vector<unsigned> ex((size_t)W), infv((size_t)W);
    for (int w = 0; w < W; ++w) {
        unsigned acc = 0u;
        for (int m = 0; m < n_mem; ++m) acc |= I.at((size_t)ro_clamp(members.at((size_t)m), 0, R - 1) * W + w);
        const unsigned valid = ro_valid(M, w);
        infv.at((size_t)w) = inf.at((size_t)w) & valid;
        ex.at((size_t)w) = ro_exon_word(acc, I.at((size_t)w), infv.at((size_t)w), valid);
    }
    std::vector<unsigned char> exons((size_t)M), e;
    for (int k = 0; 4 * k < M; ++k) {
        const unsigned v = ro_exon_bytes4(ex.at((size_t)(k >> 3)), k & 7);
        for (int b = 0; b < 4 && 4 * k + b < M; ++b) exons.at((size_t)(4 * k + b)) = (unsigned char)(v >> (8 * b));
    }
    for (int w = 0; w < W; ++w)
        for (unsigned m = infv.at((size_t)w); m; m &= m - 1) e.push_back((unsigned char)((ex.at((size_t)w) >> __builtin_ctz(m)) & 1u));
    // ---- k_readout_corr: a lane per (member, word)
    std::vector<unsigned char> corr((size_t)row_offset + (size_t)n_mem * (size_t)M, (unsigned char)'?');
    long long wide = 0, single = 0;
    for (int m = 0; m < n_mem; ++m) {
        const size_t rep = (size_t)ro_clamp(members.at((size_t)m), 0, R - 1);
        const ro_i64 row = row_offset + (ro_i64)m * M;
        for (int w = 0; w < W; ++w) {
            const int nv = ro_word_segs(M, w);
            const ro_u64 x = (ro_u64)L.at(rep * LW + (size_t)(2 * w < LW ? 2 * w : LW - 1)) | (2 * w + 1 < LW ? (ro_u64)L.at(rep * LW + 2 * w + 1) << 32 : 0ull);
            const unsigned cw = C.at(rep * W + w), iw = infv.at((size_t)w), xw = ex.at((size_t)w);
            const size_t at = (size_t)(row + 32 * w);
            const int halves = ro_store_halves((ro_u64)at, nv);
            for (int h = 0; h < 2; ++h)
                if (halves & (1 << h)) {
                    for (int k = 0; k < 4; ++k) store4(corr, at + 16 * h + 4 * k, ro_corr_bytes4(x, cw, iw, xw, 4 * h + k));
                    ++wide;
                }
            for (int b = (halves & 2) ? 32 : (halves & 1) ? 16 : 0; b < nv; ++b, ++single) corr.at(at + (size_t)b) = (unsigned char)ro_corr_byte(x, cw, iw, xw, b);
        }
    }
    for (int w = 0; w < W; ++w) printf("%s%08x", w ? " " : "", ex[(size_t)w]);
    printf("\n");
    for (unsigned char v : exons) putchar('0' + v);
    printf("\n");
    for (unsigned char v : e) putchar('0' + v);
    printf("\n");
    for (int m = 0; m < n_mem; ++m) {
        fwrite(corr.data() + row_offset + (size_t)m * M, 1, (size_t)M, stdout);
        printf("\n");
    }
    printf("%lld %lld\n", wide, single);
}

}  // namespace

int main() {
    long long M;
    while (read_int(M)) run_problem((int)M);
    return 0;
}
