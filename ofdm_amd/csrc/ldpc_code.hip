// ldpc_code.hip -- the LDPC(648) codes of OFDM_ECC_LDPC648 / _R23 / _R34 / _R56 on the host: ofdm_ldpc648_coded_len / _encode /
// _decode (rate 1/2) and ofdm_ldpc648_*_rate (rate 0 = 1/2, 1 = 2/3, 2 = 3/4, 3 = 5/6), one encoder and one decoder over
// ldpc_table.h's LdpcCode.  Parity unpinned by the reference (it has no LDPC code): tests/ldpc_ref.py and tests/ldpc_rates_ref.py
// (numpy, exact integers) are the definition, this file is its executable form in the library, and k_ldpc_encode / k_ldpc_decode
// (kernels_ldpc.hip) are held to both bit for bit.
//
// Code word of a rate, K info bytes, M = 27 * rows checks.  x[0 .. 8 K - 1] = the info bytes, each LSB first; x[8 K .. 647 - M] = 0 (shortened);
// x[648 - M .. 647] = the unique parity with H x = 0 (H: ldpc_table.h).  Sent: x[0 .. 8 K - 1] ++ the first 640 - 8 K parity bits,
// packed LSB first into 80 bytes; the parity bits behind them are punctured.  Rate 1/2: K = 40, x[320 .. 323] = 0, x[324 .. 643] sent.
//
// Decoder: layered normalised min-sum (factor 3/4) in exact integers.  Input 640 int8 LLRs a code word, positive = bit 1 (as everywhere
// in the library); inside, positive = bit 0.  Q_v = -L of a sent bit, +2047 of a shortened one, 0 of a punctured one (LdpcCode::
// llr_index); every R = 0.  Iteration it = 1, 2, ...: block rows l = 0 .. rows - 1 in order; for check z of the row with its edges e
// in table order, v_e = 27 c_e + (z + s_e) mod 27:
//     T_e = clamp(Q_{v_e} - R_e, +-2047);  m_e = min_{e' != e} |T_e'|;  sign_e = prod_{e' != e} (T_e' < 0 ? -1 : +1);
//     R_e = sign_e min((3 m_e) >> 2, 127);  Q_{v_e} = clamp(T_e + R_e, +-2047).
// After each whole iteration x_v = (Q_v < 0); if all checks hold the code word has CONVERGED at iteration it and stops, otherwise
// up to max_iter iterations run.  Output: x[0 .. 8 K - 1] of the last iteration run; iters = it when converged, 0 when not.
#include "../../include/ofdm_hip.h"
#include "ldpc_table.h"

#include <cstring>

using namespace ofdm;

namespace {

inline int clampi(int v, int lim) { return v > lim ? lim : (v < -lim ? -lim : v); }

void encode_codeword(const LdpcCode &C, const uint8_t *info, uint8_t *code) {
    const int k = C.info_cols();
    uint32_t u[kLdpcCols] = {0}, par[kLdpcRows] = {0}, lam[kLdpcRows], p0 = 0;
    for (int v = 0; v < C.info_bits(); v++)
        if ((info[v >> 3] >> (v & 7)) & 1) u[v / kLdpcZ] |= 1u << (v % kLdpcZ);
    for (int l = 0; l < C.rows; l++) {
        lam[l] = 0;
        for (int c = 0; c < k; c++)
            if (C.shift[l][c] >= 0) lam[l] ^= ldpc_rot(u[c], C.shift[l][c]);
        p0 ^= lam[l];
    }
    par[0] = p0;
    for (int l = 0; l + 1 < C.rows; l++)
        par[l + 1] = lam[l] ^ (l ? par[l] : 0u) ^ (C.shift[l][k] >= 0 ? ldpc_rot(p0, C.shift[l][k]) : 0u);
    std::memcpy(code, info, C.info_bytes);
    std::memset(code + C.info_bytes, 0, kLdpcCodeBytes - C.info_bytes);
    for (int t = 0; t < C.parity_sent(); t++) // parity bit t = x[648 - M + t]; those behind the 640 sent bits are punctured
        if ((par[t / kLdpcZ] >> (t % kLdpcZ)) & 1) code[C.info_bytes + (t >> 3)] |= (uint8_t)(1u << (t & 7));
}

// -> the iteration at which the code word converged, 0 if it did not within max_iter
int decode_codeword(const LdpcCode &C, const int8_t *llr, int max_iter, uint8_t *out) {
    int16_t Q[kLdpcN];
    int8_t R[kLdpcEdges][kLdpcZ];
    for (int v = 0; v < kLdpcN; v++) {
        const int i = C.llr_index(v);
        Q[v] = (int16_t)(i >= 0 ? -(int)llr[i] : (i == -1 ? kLdpcQMax : 0));
    }
    std::memset(R, 0, sizeof(R));
    int iters = 0;
    for (int it = 1; it <= max_iter && !iters; it++) {
        for (int l = 0; l < C.rows; l++) {
            const int e0 = C.first[l], deg = C.first[l + 1] - e0;
            for (int z = 0; z < kLdpcZ; z++) {
                int T[kLdpcCols], var[kLdpcCols];
                for (int i = 0; i < deg; i++) {
                    var[i] = kLdpcZ * C.col[e0 + i] + (z + C.sh[e0 + i]) % kLdpcZ;
                    T[i] = clampi(Q[var[i]] - R[e0 + i][z], kLdpcQMax);
                }
                for (int i = 0; i < deg; i++) {
                    int m = 1 << 30, sign = 1;
                    for (int j = 0; j < deg; j++) {
                        if (j == i) continue;
                        const int a = T[j] < 0 ? -T[j] : T[j];
                        if (a < m) m = a;
                        if (T[j] < 0) sign = -sign;
                    }
                    int r = (3 * m) >> 2;
                    if (r > kLdpcRMax) r = kLdpcRMax;
                    R[e0 + i][z] = (int8_t)(sign * r);
                    Q[var[i]] = (int16_t)clampi(T[i] + sign * r, kLdpcQMax);
                }
            }
        }
        bool ok = true;
        for (int l = 0; l < C.rows && ok; l++)
            for (int z = 0; z < kLdpcZ && ok; z++) {
                int par = 0;
                for (int e = C.first[l]; e < C.first[l + 1]; e++) par ^= Q[kLdpcZ * C.col[e] + (z + C.sh[e]) % kLdpcZ] < 0;
                ok = !par;
            }
        if (ok) iters = it;
    }
    std::memset(out, 0, C.info_bytes);
    for (int v = 0; v < C.info_bits(); v++)
        if (Q[v] < 0) out[v >> 3] |= (uint8_t)(1u << (v & 7));
    return iters;
}

} // namespace

extern "C" {

// rate 1/2 by its own names
int64_t ofdm_ldpc648_coded_len(int64_t payload_bytes) { return ofdm_ldpc648_coded_len_rate(payload_bytes, 0); }
int ofdm_ldpc648_encode(const uint8_t *info, int64_t n_cw, uint8_t *code) { return ofdm_ldpc648_encode_rate(info, n_cw, 0, code); }
int ofdm_ldpc648_decode(const int8_t *llr, int64_t n_cw, int32_t max_iter, uint8_t *out, int32_t *iters) {
    return ofdm_ldpc648_decode_rate(llr, n_cw, max_iter, 0, out, iters);
}

int32_t ofdm_ldpc648_info_bytes(int32_t rate) {
    if (rate < 0 || rate >= kLdpcRates) return OFDM_ERR_INVALID;
    return kLdpcCodes[rate].info_bytes;
}

int64_t ofdm_ldpc648_coded_len_rate(int64_t payload_bytes, int32_t rate) {
    if (payload_bytes < 0 || rate < 0 || rate >= kLdpcRates) return OFDM_ERR_INVALID;
    return kLdpcCodeBytes * ldpc_stream_codewords(payload_bytes, kLdpcCodes[rate].info_bytes);
}

int ofdm_ldpc648_encode_rate(const uint8_t *info, int64_t n_cw, int32_t rate, uint8_t *code) {
    if (rate < 0 || rate >= kLdpcRates || n_cw < 0 || (n_cw > 0 && (!info || !code))) return OFDM_ERR_INVALID;
    const LdpcCode &C = kLdpcCodes[rate];
    for (int64_t k = 0; k < n_cw; k++) encode_codeword(C, info + k * C.info_bytes, code + k * kLdpcCodeBytes);
    return OFDM_OK;
}

int ofdm_ldpc648_decode_rate(const int8_t *llr, int64_t n_cw, int32_t max_iter, int32_t rate, uint8_t *out, int32_t *iters) {
    if (rate < 0 || rate >= kLdpcRates || n_cw < 0 || max_iter < 1 || max_iter > kLdpcMaxIterLimit || (n_cw > 0 && (!llr || !out)))
        return OFDM_ERR_INVALID;
    const LdpcCode &C = kLdpcCodes[rate];
    for (int64_t k = 0; k < n_cw; k++) {
        const int it = decode_codeword(C, llr + k * kLdpcSentBits, max_iter, out + k * C.info_bytes);
        if (iters) iters[k] = it;
    }
    return OFDM_OK;
}

} // extern "C"
