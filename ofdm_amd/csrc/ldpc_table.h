// ldpc_table.h -- the one copy of the LDPC(648) codes of OFDM_ECC_LDPC648 / _R23 / _R34 / _R56, shared by the host code
// (ldpc_code.hip) and the kernels (kernels_ldpc.hip): the four shift tables, and kLdpcCodes[rate] built from them (LdpcCode: a code's
// edge list, its sent map and the check of its dual diagonal).  First the rate-1/2 table, the LDPC(648,324) code of OFDM_ECC_LDPC648;
// include/ofdm_hip.h "LDPC(648,324)" and tests/ldpc_ref.py state the same table; this one is what runs.
// Quasi-cyclic, Z = 27, 12 x 24 blocks, 88 non-zero: entry s >= 0 is the 27 x 27 identity shifted so that check z of block row l
// touches variable 27 c + (z + s) mod 27 of block column c, -1 a zero block.  Intended to be the n = 648, rate-1/2 matrix of
// 802.11n, written from memory and UNVERIFIED against the standard (as ofdm_stdrng_pilots is): the table is the definition.
#pragma once
#include <stdint.h>

namespace ofdm {

constexpr int kLdpcZ = 27, kLdpcRows = 12, kLdpcCols = 24, kLdpcEdges = 88;
constexpr int kLdpcN = kLdpcZ * kLdpcCols;                                     // 648 variables
constexpr int kLdpcCodeBytes = 80, kLdpcSentBits = 8 * kLdpcCodeBytes;         // every rate sends 640 bits of a code word
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

// bit z of the result = bit (z + s) mod 27 of the 27-bit word w: what check z of a block with shift s sees of its block column
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t ldpc_rot(uint32_t w, int s) { return s ? ((w >> s) | (w << (kLdpcZ - s))) & ((1u << kLdpcZ) - 1u) : w; }


// ---- the family: rates 1/2 (the table above), 2/3, 3/4 and 5/6 (OFDM_ECC_LDPC648_R23 / _R34 / _R56).
// The three tables below are THE PROJECT'S OWN, found by a seeded greedy search (block placement that balances the row degrees,
// shifts drawn so that no 4-cycle arises, the draw with the fewest 6-cycles of 30 kept).  They are NOT the matrices of 802.11n; the
// tables are the definition.  Same conventions as kLdpcShift; Z = 27 and 24 block columns throughout, 8 / 6 / 4 block rows.
constexpr int kLdpcRates = 4;          // rate index 0 = 1/2, 1 = 2/3, 2 = 3/4, 3 = 5/6
constexpr int kLdpcMaxRowDegree = 22;  // a row's sign bits fit one dword beside nothing else (kernels_ldpc.hip)

constexpr int8_t kLdpcShiftR23[8][kLdpcCols] = {
    {15,  5, 24, -1,  3, 14, -1, -1,  8, 23, -1,  4, -1, -1, 13, -1,  1,  0, -1, -1, -1, -1, -1, -1},
    { 5,  2, 12,  9, -1, 17, -1,  1, -1, -1, 10, -1, 26, -1, -1, -1, -1,  0,  0, -1, -1, -1, -1, -1},
    {21, 24, 22,  2, -1,  2, 25, -1,  4, -1, -1,  5, -1, -1, -1, -1, -1, -1,  0,  0, -1, -1, -1, -1},
    {26, 13,  7, 22, -1, -1, 15, -1, 11, -1, 18, -1, 17, -1, -1,  4, -1, -1, -1,  0,  0, -1, -1, -1},
    { 0,  5, -1, 15,  0, 24, -1, 11, -1, 10, -1, -1, -1,  0,  1, -1,  0, -1, -1, -1,  0,  0, -1, -1},
    { 3, 21, 18, 12, 22, -1, 25, -1, -1, 22, -1, -1, 16, -1, -1,  5, -1, -1, -1, -1, -1,  0,  0, -1},
    { 5, 14, 22,  8, -1, -1, 13, 14, -1, -1, 18, -1, -1,  2, -1, 11, -1, -1, -1, -1, -1, -1,  0,  0},
    { 4, 17,  7,  5, 26, -1, -1,  3, -1, -1, -1,  5, -1,  8, 16, -1,  1, -1, -1, -1, -1, -1, -1,  0},
};
constexpr int8_t kLdpcShiftR34[6][kLdpcCols] = {
    {11, 13, 17, 14, 16, -1, 14, 20, -1, 26, -1,  2, 26, -1, -1, 26, 23, -1,  1,  0, -1, -1, -1, -1},
    {21,  3, 11, 15, 13, 26,  5, -1, -1, 15, -1,  8, -1, 13, -1, 21, -1, 18, -1,  0,  0, -1, -1, -1},
    {22,  1, 21,  6, 21,  8, -1, 20, 25, -1, 16, -1,  9, -1, -1, 17, -1, 25, -1, -1,  0,  0, -1, -1},
    {18, 22, 11, 25, 18, 13, -1, 13, 26, -1, 22, -1, 21, -1, 16, -1,  4, -1,  0, -1, -1,  0,  0, -1},
    {13, 18,  5, 12, 20, -1,  3, 21,  0, -1, -1, 11, -1, 25,  8, -1, 19, -1, -1, -1, -1, -1,  0,  0},
    {25, 22, 21,  3, 13, 24, 10, -1, -1, 24, 12, -1, -1,  3, 10, -1, -1,  3,  1, -1, -1, -1, -1,  0},
};
constexpr int8_t kLdpcShiftR56[4][kLdpcCols] = {
    {10, 13, 21, 20, 13, 19, 12, 15,  6, 26, 10, 20,  9, -1, 11, 18, -1, 10, 19, 23,  1,  0, -1, -1},
    { 5, 21, 26, 18, 17, 12, 15, 14,  2, 18,  0,  9, -1, 23, 20, 20, 21, -1,  4,  7, -1,  0,  0, -1},
    {19, 20,  4, 22, 11,  7, 13, 11, 14, 20, 16, 17, 22, 15,  0, -1, 14, 10, -1, 13,  0, -1,  0,  0},
    {22, 15, 22, 11, 21,  3, 21, 25, 12, 19,  8, 23,  8, 22, -1, 23, 19,  4,  6, -1,  1, -1, -1,  0},
};

// One code of the family: its table (the first `rows` rows), its non-zero blocks in table order (row by row, left to right: edge e of
// block row l is first[l] <= e < first[l + 1], block column col[e], shift sh[e]) and what of a code word travels.
// x[0 .. 8 K - 1] = the K info bytes, LSB first; x[8 K .. 647 - M] = 0 (shortened, not sent), M = 27 rows; x[648 - M .. 647] = the
// parity.  Sent, 640 bits: x[0 .. 8 K - 1] ++ x[648 - M .. 648 - M + (640 - 8 K) - 1]; the parity bits behind them are punctured.
struct LdpcCode {
    int rows, info_bytes, count, max_degree;
    int8_t shift[kLdpcRows][kLdpcCols];
    uint8_t col[kLdpcEdges], sh[kLdpcEdges], first[kLdpcRows + 1];
    constexpr int checks() const { return kLdpcZ * rows; }
    constexpr int info_cols() const { return kLdpcCols - rows; }
    constexpr int info_bits() const { return 8 * info_bytes; }
    constexpr int first_parity() const { return kLdpcN - kLdpcZ * rows; }
    constexpr int parity_sent() const { return kLdpcSentBits - 8 * info_bytes; }
    // where variable v starts from: the index of its LLR among the 640, -1 shortened (+kLdpcQMax), -2 punctured (0)
    constexpr int llr_index(int v) const {
        if (v < info_bits()) return v;
        if (v < first_parity()) return -1;
        return v < first_parity() + parity_sent() ? v - first_parity() + info_bits() : -2;
    }
    // The parity part is dual-diagonal behind column k = info_cols(): block column k + j (j >= 1) has the unshifted identity in rows
    // j - 1 and j and nothing else, column k has three blocks (rows 0, rows / 2 and rows - 1) whose first and last shifts agree and
    // whose middle one is unshifted.  Summed over the rows every column from k + 1 on cancels and column k leaves its middle block, so
    // with lambda_l the info part of row l:  p_0 = xor_l lambda_l, then p_{l+1} = lambda_l ^ p_l [l > 0] ^ rot(p_0, shift of column k
    // in row l), l = 0 .. rows - 2.
    constexpr bool dual_diagonal() const {
        const int k = info_cols();
        for (int l = 0; l < rows; l++)
            for (int j = 1; j < rows; j++)
                if (shift[l][k + j] != ((l == j - 1 || l == j) ? 0 : -1)) return false;
        for (int l = 0; l < rows; l++)
            if ((shift[l][k] >= 0) != (l == 0 || l == rows / 2 || l == rows - 1)) return false;
        return shift[0][k] == shift[rows - 1][k] && shift[rows / 2][k] == 0;
    }
};
template <int R>
constexpr LdpcCode make_ldpc_code(const int8_t (&table)[R][kLdpcCols], int info_bytes) {
    LdpcCode t{};
    t.rows = R; t.info_bytes = info_bytes;
    int e = 0;
    for (int l = 0; l < kLdpcRows; l++) {
        t.first[l] = (uint8_t)e;
        for (int c = 0; c < kLdpcCols; c++) {
            t.shift[l][c] = l < R ? table[l][c] : (int8_t)-1;
            if (t.shift[l][c] >= 0) {
                if (e < kLdpcEdges) { t.col[e] = (uint8_t)c; t.sh[e] = (uint8_t)t.shift[l][c]; }
                e++;
            }
        }
        if (e - t.first[l] > t.max_degree) t.max_degree = e - t.first[l];
    }
    t.first[kLdpcRows] = (uint8_t)e;
    t.count = e;
    return t;
}
constexpr LdpcCode kLdpcCodes[kLdpcRates] = {make_ldpc_code(kLdpcShift, 40), make_ldpc_code(kLdpcShiftR23, 53),
                                             make_ldpc_code(kLdpcShiftR34, 60), make_ldpc_code(kLdpcShiftR56, 67)};
static_assert(kLdpcCodes[0].count == 88 && kLdpcCodes[1].count == 87 && kLdpcCodes[2].count == 85 && kLdpcCodes[3].count == 81,
              "the non-zero blocks of the four tables");
static_assert(kLdpcCodes[0].dual_diagonal() && kLdpcCodes[1].dual_diagonal() && kLdpcCodes[2].dual_diagonal() && kLdpcCodes[3].dual_diagonal(),
              "the encoders back-substitute along the dual diagonal");
static_assert(kLdpcCodes[0].max_degree == 8 && kLdpcCodes[1].max_degree == 12 && kLdpcCodes[2].max_degree == 15 && kLdpcCodes[3].max_degree == 21 &&
              kLdpcCodes[3].max_degree <= kLdpcMaxRowDegree, "row degrees");
static_assert(kLdpcCodes[1].info_bits() <= kLdpcCodes[1].first_parity() && kLdpcCodes[2].info_bits() <= kLdpcCodes[2].first_parity() &&
              kLdpcCodes[3].info_bits() <= kLdpcCodes[3].first_parity() && kLdpcCodes[1].parity_sent() <= kLdpcCodes[1].checks() &&
              kLdpcCodes[2].parity_sent() <= kLdpcCodes[2].checks() && kLdpcCodes[3].parity_sent() <= kLdpcCodes[3].checks(),
              "640 sent bits: the info bits and a prefix of the parity");
static_assert(kLdpcCodes[0].llr_index(319) == 319 && kLdpcCodes[0].llr_index(320) == -1 && kLdpcCodes[0].llr_index(324) == 320 &&
              kLdpcCodes[0].llr_index(643) == 639 && kLdpcCodes[0].llr_index(644) == -2, "rate 1/2 keeps its sent map");

// codewords of p payload bytes behind the two length words, K info bytes a code word
constexpr int64_t ldpc_stream_codewords(int64_t p, int k) { return (p + 8 + k - 1) / k; }

} // namespace ofdm
