// clu_readout.h -- what one thread of the round read-out (fclu_round_readout; k_readout_exons / k_readout_corr in freddie_cluster.hip) computes
// for one 32-bit word of a row: the isoform's exon word from the members' I words, its expansion to bytes, and the 32 correction characters
// of a member from its label words, its C word, the informative word and the exon word.  Host and device: tools/readout_host_check.cpp runs
// the same functions over whole rows and is compared word by word with the numpy mirror (cluster_prep.readout_mirror) where there is no GPU.
// The definition is cluster.read_out() (run_ilp's read-out, py/freddie_cluster.py:601-635).
//
// A row of M segments is W = max(ceil(M / 32), 1) bit words (bit j & 31 of word j >> 5 = segment j) and LW = max(ceil(M / 16), 1) label
// words at two bits a label (fclu_reads): bit word w belongs to the label words 2 w and 2 w + 1.  Bytes are packed four to a word with
// segment 4 k at the lowest address (little endian), so that a lane stores 16 of them at once where the address allows.  Nothing here
// indexes memory: the callers clamp what they read.
#ifndef CLU_READOUT_H
#define CLU_READOUT_H

#include <stdint.h>

#if defined(__HIPCC__)
#define RO_HD __host__ __device__ __forceinline__
#else
#define RO_HD inline
#endif

typedef long long ro_i64;
typedef unsigned long long ro_u64;

RO_HD ro_i64 ro_clamp(ro_i64 v, ro_i64 lo, ro_i64 hi) { return v < lo ? lo : v > hi ? hi : v; }

// the segments of word w inside a row of M: 32, fewer in the last word, none behind it
RO_HD int ro_word_segs(int M, int w) { const ro_i64 n = (ro_i64)M - 32ll * w; return n >= 32 ? 32 : n <= 0 ? 0 : (int)n; }
RO_HD unsigned ro_valid(int M, int w) { const int n = ro_word_segs(M, w); return n >= 32 ? 0xffffffffu : (1u << n) - 1u; }

// The exon word: on an informative segment the OR of the members' I bits (e), elsewhere the I bit of column 0 of the problem, member or
// not (read_out's e_of rule); the bits behind M are cut.
RO_HD unsigned ro_exon_word(unsigned member_or, unsigned col0, unsigned inf, unsigned valid) { return ((member_or & inf) | (col0 & ~inf)) & valid; }

// bits 4 k .. 4 k + 3 of a word as four bytes 0 / 1
RO_HD unsigned ro_exon_bytes4(unsigned ex, int k) {
    const unsigned n = (ex >> (4 * (k & 7))) & 0xfu;
    return (n & 1u) | ((n & 2u) << 7) | ((n & 4u) << 14) | ((n & 8u) << 21);
}

// One correction character, bit b of the word: '-' on an uninformative segment, 'X' where the member's C bit and the exon bit are both 1,
// otherwise the label's own digit.  lab: the label words 2 w (low half) and 2 w + 1 (high half), two bits a label.
RO_HD unsigned ro_corr_byte(ro_u64 lab, unsigned cb, unsigned inf, unsigned ex, int b) {
    b &= 31;
    if (!((inf >> b) & 1u)) return (unsigned)'-';
    if ((cb >> b) & (ex >> b) & 1u) return (unsigned)'X';
    return (unsigned)'0' + (unsigned)((lab >> (2 * b)) & 3ull);
}

// the characters of bits 4 k .. 4 k + 3, packed
RO_HD unsigned ro_corr_bytes4(ro_u64 lab, unsigned cb, unsigned inf, unsigned ex, int k) {
    const int b = 4 * (k & 7);
    return ro_corr_byte(lab, cb, inf, ex, b) | (ro_corr_byte(lab, cb, inf, ex, b + 1) << 8) | (ro_corr_byte(lab, cb, inf, ex, b + 2) << 16) |
           (ro_corr_byte(lab, cb, inf, ex, b + 3) << 24);
}

// How a lane writes the n (0 .. 32) bytes of its word at byte address a: the 16-byte halves it may store whole -- the address is a
// multiple of 16 and the half lies inside n -- as bits 0 and 1; every other byte is stored alone.
RO_HD int ro_store_halves(ro_u64 a, int n) { return (a & 15ull) ? 0 : (n >= 16 ? 1 : 0) | (n >= 32 ? 2 : 0); }

#endif
