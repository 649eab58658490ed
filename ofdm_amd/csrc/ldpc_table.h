// ldpc_table.h -- the one copy of the LDPC(648,324) code of OFDM_ECC_LDPC648, shared by the host code (ldpc_code.hip) and the
// kernels (kernels_ldpc.hip).  include/ofdm_hip.h "LDPC(648,324)" and tests/ldpc_ref.py state the same table; this one is what runs.
// Quasi-cyclic, Z = 27, 12 x 24 blocks, 88 non-zero: entry s >= 0 is the 27 x 27 identity shifted so that check z of block row l
// touches variable 27 c + (z + s) mod 27 of block column c, -1 a zero block.  Intended to be the n = 648, rate-1/2 matrix of
// 802.11n, written from memory and UNVERIFIED against the standard (as ofdm_stdrng_pilots is): the table is the definition.
#pragma once
#include <stdint.h>

namespace ofdm {

constexpr int kLdpcZ = 27, kLdpcRows = 12, kLdpcCols = 24, kLdpcEdges = 88;
constexpr int kLdpcN = kLdpcZ * kLdpcCols, kLdpcChecks = kLdpcZ * kLdpcRows;   // 648 variables, 324 checks
constexpr int kLdpcInfoBytes = 40, kLdpcCodeBytes = 80;                        // 320 info bits, 320 info + 320 parity bits sent
constexpr int kLdpcInfoBits = 8 * kLdpcInfoBytes, kLdpcSentBits = 8 * kLdpcCodeBytes;
constexpr int kLdpcQMax = 2047, kLdpcRMax = 127;                               // clamps of the decoder's posteriors and check messages
constexpr int kLdpcMaxIterLimit = 64;

constexpr int8_t kLdpcShift[kLdpcRows][kLdpcCols] = {
    { 0, -1, -1, -1,  0,  0, -1, -1,  0, -1, -1,  0,  1,  0, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {22,  0, -1, -1, 17, -1,  0,  0, 12, -1, -1, -1, -1,  0,  0, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 6, -1,  0, -1, 10, -1, -1, -1, 24, -1,  0, -1, -1, -1,  0,  0, -1, -1, -1, -1, -1, -1, -1, -1},
    { 2, -1, -1,  0, 20, -1, -1, -1, 25,  0, -1, -1, -1, -1, -1,  0,  0, -1, -1, -1, -1, -1, -1, -1},
    {23, -1, -1, -1,  3, -1, -1, -1,  0, -1,  9, 11, -1, -1, -1, -1,  0,  0, -1, -1, -1, -1, -1, -1},
    {24, -1, 23,  1, 17, -1,  3, -1, 10, -1, -1, -1, -1, -1, -1, -1, -1,  0,  0, -1, -1, -1, -1, -1},
    {25, -1, -1, -1,  8, -1, -1, -1,  7, 18, -1, -1,  0, -1, -1, -1, -1, -1,  0,  0, -1, -1, -1, -1},
    {13, 24, -1, -1,  0, -1,  8, -1,  6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,  0,  0, -1, -1, -1},
    { 7, 20, -1, 16, 22, 10, -1, -1, 23, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,  0,  0, -1, -1},
    {11, -1, -1, -1, 19, -1, -1, -1, 13, -1,  3, 17, -1, -1, -1, -1, -1, -1, -1, -1, -1,  0,  0, -1},
    {25, -1,  8, -1, 23, 18, -1, 14,  9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,  0,  0},
    { 3, -1, -1, -1, 16, -1, -1,  2, 25,  5, -1, -1,  1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,  0},
};

// the non-zero blocks in table order (row by row, left to right): edge e of block row l is first[l] <= e < first[l + 1]
struct LdpcEdgeList {
    uint8_t col[kLdpcEdges], shift[kLdpcEdges], first[kLdpcRows + 1];
    int count;
};
constexpr LdpcEdgeList make_ldpc_edges() {
    LdpcEdgeList t{};
    int e = 0;
    for (int l = 0; l < kLdpcRows; l++) {
        t.first[l] = (uint8_t)e;
        for (int c = 0; c < kLdpcCols; c++)
            if (kLdpcShift[l][c] >= 0) {
                if (e < kLdpcEdges) { t.col[e] = (uint8_t)c; t.shift[e] = (uint8_t)kLdpcShift[l][c]; }
                e++;
            }
    }
    t.first[kLdpcRows] = (uint8_t)e;
    t.count = e;
    return t;
}
constexpr LdpcEdgeList kLdpcEdgeList = make_ldpc_edges();
static_assert(kLdpcEdgeList.count == kLdpcEdges, "88 non-zero blocks");

// The parity half is dual-diagonal behind column 12: block column 12 + j (j >= 1) has the unshifted identity in rows j - 1 and j and
// nothing else, column 12 has three blocks whose first and last shifts agree.  Summed over the rows every column from 13 on cancels
// and column 12 leaves its middle block, so with lambda_l the info part of row l:  p_0 = rot(xor_l lambda_l, -middle shift), then
// p_{l+1} = lambda_l ^ p_l [l > 0] ^ rot(p_0, shift of column 12 in row l), l = 0 .. 10.
constexpr bool ldpc_parity_is_dual_diagonal() {
    for (int l = 0; l < kLdpcRows; l++)
        for (int j = 1; j < kLdpcRows; j++)
            if (kLdpcShift[l][kLdpcRows + j] != ((l == j - 1 || l == j) ? 0 : -1)) return false;
    int n = 0, s[3] = {0, 0, 0};
    for (int l = 0; l < kLdpcRows; l++)
        if (kLdpcShift[l][kLdpcRows] >= 0) { if (n < 3) s[n] = kLdpcShift[l][kLdpcRows]; n++; }
    return n == 3 && s[0] == s[2] && s[1] == 0 && kLdpcShift[0][kLdpcRows] >= 0 && kLdpcShift[kLdpcRows - 1][kLdpcRows] >= 0;
}
static_assert(ldpc_parity_is_dual_diagonal(), "the encoders back-substitute along the dual diagonal");

// bit z of the result = bit (z + s) mod 27 of the 27-bit word w: what check z of a block with shift s sees of its block column
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t ldpc_rot(uint32_t w, int s) { return s ? ((w >> s) | (w << (kLdpcZ - s))) & ((1u << kLdpcZ) - 1u) : w; }

// codewords of p payload bytes behind the two length words
constexpr int64_t ldpc_stream_codewords(int64_t p) { return (p + 8 + kLdpcInfoBytes - 1) / kLdpcInfoBytes; }

} // namespace ofdm
