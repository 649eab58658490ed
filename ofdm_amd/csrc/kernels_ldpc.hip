// kernels_ldpc.hip -- the LDPC(648) codes of rates 1/2, 2/3, 3/4 and 5/6 on the device (OFDM_ECC_LDPC648 / _R23 / _R34 / _R56,
// ofdm_ldpc648_encode_batch / _decode_batch, their _rate_batch forms and the modes' frame chain; include/ofdm_hip.h "LDPC(648,324)"
// and "LDPC(648), rates 2/3, 3/4 and 5/6").  The codes and the decoding rule are those of ldpc_table.h (LdpcCode)
// / ldpc_code.hip / tests/ldpc_ref.py / tests/ldpc_rates_ref.py, which the kernels are held to bit for bit, iteration counts included.
// One template over the rate index, 0 = 1/2 .. 3 = 5/6; the dispatch names are k_ldpc_decode, k_ldpc_decode<r23|r34|r56> and likewise
// for the encoder.
//   k_ldpc_decode<RATE>  one wavefront per frame, four to a workgroup, persistent grid.  The wavefront takes its frame's code words two
//                  at a time: lanes 0 .. 26 and 32 .. 58, lane = check z of ALL block rows of the code.  The 648 posteriors Q of a code
//                  word sit in a slab of LDS owned by the half-wavefront (int16; the two slabs 32 banks apart), so a block row reads and
//                  writes 27 consecutive int16 per block apart from the wrap, and nothing needs a barrier: one wavefront's LDS
//                  accesses are ordered.  The check messages R_e of a lane are not stored one by one: after a row's update every
//                  R_e is sign_e times one of TWO magnitudes (min((3 m) >> 2, 127) of the smallest |T| for every edge but the one
//                  that holds it, of the second smallest for that one), so a row keeps both magnitudes, the position of the smallest
//                  and its sign bits (RowState): ONE dword at rate 1/2, whose rows have at most eight edges -- twelve VGPRs instead of
//                  88, the same integers --, TWO for the 10 .. 21 edges of the others (16 / 12 / 8 VGPRs a code).
//                  After an iteration lane z reads Q[27 c + z] for the 24 block columns; one ballot a column gives both halves'
//                  27-bit words of hard decisions in scalar registers, and the checks are rotate-xors on them in scalar code.
//                  A converged half is masked off while the other goes on.  A code word has 40 .. 67 info bytes, so a lane extracts
//                  byte `lane` and, at rate 5/6, lanes 0 .. 2 bytes 64 .. 66 as well.  The frame's verdict, length and status are
//                  wave-uniform: lane 0 writes them, no atomics, no second launch.
//   k_ldpc_encode<RATE>  one thread per code word: the 12 / 16 / 18 / 20 27-bit info words, lambda_l by rotate-xor, back-substitution
//                  along the dual diagonal (ldpc_table.h).  Chain mode builds the info stream [u32 LE p][u32 LE ~p] ++ payload on the fly.
#include "device_common.hpp"
#include "kernels.hpp"
#include "ldpc_table.h"

#include <utility>

namespace ofdm {

namespace {
constexpr int kSlab = 704; // int16 between the two slabs of a wavefront: 648 rounded up to 352 dwords = 32 banks (mod 64) apart

template <int RATE> struct Code {
    static_assert(RATE >= 0 && RATE < kLdpcRates, "rate index 0 = 1/2 .. 3 = 5/6");
    static constexpr int rows = kLdpcCodes[RATE].rows, K = kLdpcCodes[RATE].info_bytes, info_cols = kLdpcCols - rows;
    static constexpr int info_bits = 8 * K, first_parity = kLdpcN - kLdpcZ * rows, parity_sent = kLdpcSentBits - info_bits;
    static constexpr int byte_slots = (K + 63) / 64; // info bytes a lane extracts
    static constexpr bool one_dword = kLdpcCodes[RATE].max_degree <= 8; // a row's messages fit one dword (RowStates)
    static constexpr int shift(int l, int c) { return kLdpcCodes[RATE].shift[l][c]; }
    using Rows = std::make_integer_sequence<int, rows>;
    using InfoCols = std::make_integer_sequence<int, info_cols>;
};
template <int RATE, int E> struct Edge {
    static constexpr int col = kLdpcCodes[RATE].col[E], shift = kLdpcCodes[RATE].sh[E];
    // variable index of check z
    __device__ __forceinline__ static int var(int z) {
        if (shift == 0) return kLdpcZ * col + z;
        const int t = z + shift;
        return kLdpcZ * col + (t >= kLdpcZ ? t - kLdpcZ : t);
    }
};
template <int RATE, int L> struct Row {
    static constexpr int first = kLdpcCodes[RATE].first[L], degree = kLdpcCodes[RATE].first[L + 1] - kLdpcCodes[RATE].first[L];
    static_assert(degree >= 2 && degree <= (Code<RATE>::one_dword ? 8 : kLdpcMaxRowDegree), "a row's sign bits are packed beside or into one dword");
    using Edges = std::make_integer_sequence<int, degree>;
};

__device__ __forceinline__ int clamp_q(int v) { return v > kLdpcQMax ? kLdpcQMax : (v < -kLdpcQMax ? -kLdpcQMax : v); }
__device__ __forceinline__ int scale_r(int m) { const int r = (3 * m) >> 2; return r > kLdpcRMax ? kLdpcRMax : r; }

// The messages of a check's block rows.  Row l: bits 0 .. 6 of mag[l] the magnitude of every edge but one, 7 .. 13 the magnitude of
// edge where(l); bit i of signs(l) the sign of edge i (1 = negative).  All 0 = every R is 0.  Only the bit layout depends on the
// code's largest degree: two dwords a row, the position in bits 14 .. 18 of mag[l] and the signs in sg[l] ...
template <int ROWS, bool ONE_DWORD> struct RowStates {
    unsigned sg[ROWS], mag[ROWS];
    __device__ __forceinline__ int where(int l) const { return (int)((mag[l] >> 14) & 31u); }
    __device__ __forceinline__ unsigned signs(int l) const { return sg[l]; }
    __device__ __forceinline__ void set(int l, int n1, int n2, int where, unsigned sgn) {
        mag[l] = (unsigned)n1 | ((unsigned)n2 << 7) | ((unsigned)where << 14);
        sg[l] = sgn;
    }
};
// ... or, for at most eight edges, one: the position in bits 14 .. 16, the signs in bits 17 .. 24
template <int ROWS> struct RowStates<ROWS, true> {
    unsigned mag[ROWS];
    __device__ __forceinline__ int where(int l) const { return (int)((mag[l] >> 14) & 7u); }
    __device__ __forceinline__ unsigned signs(int l) const { return mag[l] >> 17; }
    __device__ __forceinline__ void set(int l, int n1, int n2, int where, unsigned sgn) {
        mag[l] = (unsigned)n1 | ((unsigned)n2 << 7) | ((unsigned)where << 14) | (sgn << 17);
    }
};
template <int RATE> using States = RowStates<Code<RATE>::rows, Code<RATE>::one_dword>;

// One block row for check z
template <int RATE, int L, int... I>
__device__ __forceinline__ void row_update(int16_t *Q, int z, States<RATE> &st, std::integer_sequence<int, I...>) {
    constexpr int e0 = Row<RATE, L>::first, deg = sizeof...(I);
    const int a1 = (int)(st.mag[L] & 127u), a2 = (int)((st.mag[L] >> 7) & 127u), at = st.where(L);
    const unsigned sg = st.signs(L);
    int var[deg], T[deg];
    ((var[I] = Edge<RATE, e0 + I>::var(z)), ...);
    ((T[I] = clamp_q((int)Q[var[I]] - (((sg >> I) & 1u) ? -(I == at ? a2 : a1) : (I == at ? a2 : a1)))), ...);
    int m1 = 4096, m2 = 4096, where = 0;
    unsigned neg = 0;
    auto track = [&](int i, int t) __attribute__((always_inline)) {
        const int a = t < 0 ? -t : t;
        where = a < m1 ? i : where;
        m2 = min(m2, max(a, m1));
        m1 = min(m1, a);
        neg |= (t < 0 ? 1u : 0u) << i;
    };
    (track(I, T[I]), ...);
    const int n1 = scale_r(m1), n2 = scale_r(m2);
    const unsigned flip = (__popc(neg) & 1) ? (1u << deg) - 1u : 0u;
    const unsigned sgn = neg ^ flip; // sign_e = the product over the OTHER edges
    ((Q[var[I]] = (int16_t)clamp_q(T[I] + (((sgn >> I) & 1u) ? -(I == where ? n2 : n1) : (I == where ? n2 : n1)))), ...);
    st.set(L, n1, n2, where, sgn);
}
template <int RATE, int... L>
__device__ __forceinline__ void iteration(int16_t *Q, int z, States<RATE> &st, std::integer_sequence<int, L...>) {
    ((row_update<RATE, L>(Q, z, st, typename Row<RATE, L>::Edges{}), wave_fence()), ...);
}

// bit z = the parity of check z of block row L over the hard-decision words w[c] of the block columns
template <int RATE, int L, int... I>
__device__ __forceinline__ unsigned row_syndrome(const unsigned (&w)[kLdpcCols], std::integer_sequence<int, I...>) {
    constexpr int e0 = Row<RATE, L>::first;
    return (ldpc_rot(w[Edge<RATE, e0 + I>::col], Edge<RATE, e0 + I>::shift) ^ ...);
}
template <int RATE, int... L>
__device__ __forceinline__ unsigned syndrome(const unsigned (&w)[kLdpcCols], std::integer_sequence<int, L...>) {
    return (row_syndrome<RATE, L>(w, typename Row<RATE, L>::Edges{}) | ...);
}

// the posteriors a code word starts from (LdpcCode::llr_index), all 64 lanes
template <int RATE>
__device__ __forceinline__ void load(const int8_t *llr, int16_t *Q, int lane) {
    using C = Code<RATE>;
#pragma unroll
    for (int v0 = 0; v0 < kLdpcN; v0 += 64) {
        const int v = v0 + lane;
        if (v < kLdpcN) {
            const bool info = v < C::info_bits, sent = info || (v >= C::first_parity && v < C::first_parity + C::parity_sent);
            const int l = sent ? (int)llr[info ? v : v - C::first_parity + C::info_bits] : 0;
            Q[v] = (int16_t)(sent ? -l : (v < C::first_parity ? kLdpcQMax : 0));
        }
    }
}

template <int RATE> struct Pair {
    int it_a, it_b;                                    // the iteration at which each code word converged, 0 = not (wave-uniform)
    unsigned byte_a[Code<RATE>::byte_slots], byte_b[Code<RATE>::byte_slots]; // slot j, lane + 64 j < K: info byte lane + 64 j of each
};
// Decodes code word A (640 LLRs at llr_a) and, if llr_b is not null, code word B beside it.  slab: the wavefront's 2 * kSlab int16.
template <int RATE>
__device__ __forceinline__ Pair<RATE> decode_pair(const int8_t *llr_a, const int8_t *llr_b, int max_iter, int16_t *slab, int lane) {
    using C = Code<RATE>;
    const bool have_b = llr_b != nullptr; // (wave-uniform)
    load<RATE>(llr_a, slab, lane);
    if (have_b) load<RATE>(llr_b, slab + kSlab, lane);
    wave_fence();
    const int z = lane & 31;
    const bool upper = lane >= 32, check = z < kLdpcZ;
    int16_t *Q = slab + (upper ? kSlab : 0);
    States<RATE> st;
#pragma unroll
    for (int l = 0; l < C::rows; ++l) st.set(l, 0, 0, 0, 0u);
    bool done_a = false, done_b = !have_b;
    Pair<RATE> r;
    r.it_a = 0; r.it_b = 0;
    for (int it = 1; it <= max_iter; ++it) {
        if (check && !(upper ? done_b : done_a)) iteration<RATE>(Q, z, st, typename C::Rows{});
        wave_fence();
        unsigned wa[kLdpcCols], wb[kLdpcCols];
#pragma unroll
        for (int c = 0; c < kLdpcCols; ++c) {
            const int q = check ? (int)Q[kLdpcZ * c + z] : 0;
            const unsigned long long b = __ballot(q < 0);
            wa[c] = (unsigned)b;
            wb[c] = (unsigned)(b >> 32);
        }
        if (!done_a && syndrome<RATE>(wa, typename C::Rows{}) == 0) { done_a = true; r.it_a = it; }
        if (!done_b && syndrome<RATE>(wb, typename C::Rows{}) == 0) { done_b = true; r.it_b = it; }
        if (done_a && done_b) break;
    }
#pragma unroll
    for (int j = 0; j < C::byte_slots; ++j) {
        r.byte_a[j] = 0; r.byte_b[j] = 0;
        const int i = lane + 64 * j;
        if (i < C::K) {
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                r.byte_a[j] |= (slab[8 * i + b] < 0 ? 1u : 0u) << b;
                r.byte_b[j] |= (slab[kSlab + 8 * i + b] < 0 ? 1u : 0u) << b;
            }
        }
    }
    wave_fence(); // the next pair's load overwrites the slabs
    return r;
}
// info bytes `from` .. K - 1 of one code word of a pair to row[at + from .. at + K - 1]
template <int RATE>
__device__ __forceinline__ void store_bytes(uint8_t *row, long long at, const unsigned (&bytes)[Code<RATE>::byte_slots], int lane, int from = 0) {
#pragma unroll
    for (int j = 0; j < Code<RATE>::byte_slots; ++j) {
        const int i = lane + 64 * j;
        if (i >= from && i < Code<RATE>::K) row[at + i] = (uint8_t)bytes[j];
    }
}
__device__ __forceinline__ unsigned word_le(unsigned bytes, int first) { // the u32 in lanes first .. first + 3
    unsigned w = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) w |= ((unsigned)__builtin_amdgcn_readlane((int)bytes, first + i) & 0xFFu) << (8 * i);
    return w;
}
} // namespace

// Stage mode (status_rw == nullptr): row f holds n_cw code words of 640 LLRs; K n_cw bytes out, iters[f * n_cw + k] (optional).
// Chain mode (the frame modes): body = the demodulated bytes behind the 16-byte header (not read), nb = body / 80 whole code words
// from LLR 128 on.  nb = 0, code word 0 unconverged or its bytes 4 .. 7 not the complement of bytes 0 .. 3: status OFDM_FRAME_HEADER.
// Else with p = bytes 0 .. 3 and B = ceil((p + 8) / K) the code words 1 .. min(B, nb) - 1 are decoded; one unconverged: status
// OFDM_FRAME_UNCORRECTABLE; else min(p, K nb - 8) bytes of the stream behind the two length words are delivered.
template <int RATE>
__global__ __launch_bounds__(256) void k_ldpc_decode(LdpcDecodeParams p) {
    constexpr int K = Code<RATE>::K;
    __shared__ __attribute__((aligned(16))) int16_t q_lds[4][2 * kSlab];
    const int lane = threadIdx.x & 63;
    int16_t *slab = q_lds[threadIdx.x >> 6];
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (long long)gridDim.x * 4;
    for (long long f = wave; f < p.n_frames; f += n_waves) {
        const int8_t *l = p.llr + f * p.llr_stride;
        uint8_t *dst = p.out + f * p.out_stride;
        if (!p.status_rw) {
            for (long long k = 0; k < p.n_cw; k += 2) {
                const bool two = k + 1 < p.n_cw;
                const Pair<RATE> r = decode_pair<RATE>(l + k * kLdpcSentBits, two ? l + (k + 1) * kLdpcSentBits : nullptr, p.max_iter, slab, lane);
                store_bytes<RATE>(dst, k * K, r.byte_a, lane);
                if (two) store_bytes<RATE>(dst, (k + 1) * K, r.byte_b, lane);
                if (p.iters && lane == 0) {
                    p.iters[f * p.n_cw + k] = r.it_a;
                    if (two) p.iters[f * p.n_cw + k + 1] = r.it_b;
                }
            }
            continue;
        }
        if (__builtin_amdgcn_readfirstlane(p.status_rw[f]) != 0) { if (lane == 0) p.out_len[f] = 0; continue; }
        const long long body = (long long)__builtin_amdgcn_readfirstlane(p.nsym[f]) * p.bytes_per_symbol - 16;
        const long long nb = body > 0 ? body / kLdpcCodeBytes : 0;
        l += 128;
        int status = 0;
        long long n_out = 0;
        if (nb == 0) status = -4; // OFDM_FRAME_HEADER
        else {
            const Pair<RATE> h = decode_pair<RATE>(l, nb >= 2 ? l + kLdpcSentBits : nullptr, p.max_iter, slab, lane);
            const unsigned len = word_le(h.byte_a[0], 0), inv = word_le(h.byte_a[0], 4);
            if (h.it_a == 0 || inv != ~len) status = -4;
            else {
                const long long want = (long long)(((unsigned long long)len + 8u + K - 1) / K);
                const long long n_cw = want < nb ? want : nb;
                bool bad = n_cw >= 2 && h.it_b == 0;
                if (!bad) { // the stream behind the two length words: byte i of code word k is dst[k K - 8 + i]
                    store_bytes<RATE>(dst, -8, h.byte_a, lane, 8);
                    if (n_cw >= 2) store_bytes<RATE>(dst, K - 8, h.byte_b, lane);
                }
                for (long long k = 2; k < n_cw && !bad; k += 2) {
                    const bool two = k + 1 < n_cw;
                    const Pair<RATE> r = decode_pair<RATE>(l + k * kLdpcSentBits, two ? l + (k + 1) * kLdpcSentBits : nullptr, p.max_iter, slab, lane);
                    bad = r.it_a == 0 || (two && r.it_b == 0);
                    if (!bad) {
                        store_bytes<RATE>(dst, k * K - 8, r.byte_a, lane);
                        if (two) store_bytes<RATE>(dst, (k + 1) * K - 8, r.byte_b, lane);
                    }
                }
                const long long room = (long long)K * nb - 8;
                if (bad) status = -5; // OFDM_FRAME_UNCORRECTABLE
                else n_out = (long long)len < room ? (long long)len : room;
            }
        }
        if (lane == 0) {
            if (status) p.status_rw[f] = status;
            p.out_len[f] = (int32_t)n_out;
        }
    }
}

namespace {
template <int RATE, int L, int... C>
__device__ __forceinline__ unsigned lambda(const unsigned (&u)[Code<RATE>::info_cols], std::integer_sequence<int, C...>) {
    return ((Code<RATE>::shift(L, C) >= 0 ? ldpc_rot(u[C], Code<RATE>::shift(L, C) >= 0 ? Code<RATE>::shift(L, C) : 0) : 0u) ^ ...);
}
template <int RATE, int... L>
__device__ __forceinline__ void parity(const unsigned (&u)[Code<RATE>::info_cols], unsigned (&par)[Code<RATE>::rows], std::integer_sequence<int, L...>) {
    constexpr int rows = Code<RATE>::rows, k = Code<RATE>::info_cols;
    unsigned lam[rows];
    ((lam[L] = lambda<RATE, L>(u, typename Code<RATE>::InfoCols{})), ...);
    const unsigned p0 = (lam[L] ^ ...);
    par[0] = p0;
    ((L + 1 < rows
          ? (void)(par[L + 1 < rows ? L + 1 : 0] =
                       lam[L] ^ (L ? par[L] : 0u) ^ (Code<RATE>::shift(L, k) >= 0 ? ldpc_rot(p0, Code<RATE>::shift(L, k) >= 0 ? Code<RATE>::shift(L, k) : 0) : 0u))
          : (void)0),
     ...);
}
} // namespace

// One code word per thread.  Stage mode (framed == 0): row f = n_cw blocks of K info bytes -> n_cw blocks of 80 code bytes.
// Chain mode: row f = len_f payload bytes (in_len[f] clamped to [0, n_bytes], or n_bytes) -> the code of the info stream [u32 LE
// len_f][u32 LE ~len_f] ++ payload, zero-padded to ceil((len_f + 8) / K) code words; the code words behind them, up to n_cw, are
// written as zeros; out_len[f] (optional) = 80 ceil((len_f + 8) / K).
template <int RATE>
__global__ __launch_bounds__(256) void k_ldpc_encode(LdpcEncodeParams p) {
    using C = Code<RATE>;
    constexpr int K = C::K;
    const long long units = p.n_frames * p.n_cw;
    for (long long u = (long long)blockIdx.x * 256 + threadIdx.x; u < units; u += (long long)gridDim.x * 256) {
        const long long f = u / p.n_cw, k = u - f * p.n_cw;
        const uint8_t *src = p.in + f * p.in_stride;
        uint8_t *dst = p.out + f * p.out_stride + k * kLdpcCodeBytes;
        long long len = p.n_bytes;
        if (p.framed) {
            if (p.in_len) { const long long v = p.in_len[f]; len = v < 0 ? 0 : (v > p.n_bytes ? p.n_bytes : v); }
            const long long own = ldpc_stream_codewords(len, K);
            if (k == 0 && p.out_len) p.out_len[f] = (int32_t)(kLdpcCodeBytes * own);
            if (k >= own) {
                for (int i = 0; i < kLdpcCodeBytes; ++i) dst[i] = 0;
                continue;
            }
        }
        unsigned w[C::info_cols], par[C::rows];
        unsigned long long acc = 0;
        int have = 0, nw = 0;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            unsigned b;
            if (p.framed) {
                const long long i = k * K + j;
                const unsigned word = i < 4 ? (unsigned)len : ~(unsigned)len;
                b = i < 8 ? (word >> (8 * (i & 3))) & 0xFFu : (i - 8 < len ? (unsigned)src[i - 8] : 0u);
            } else b = src[k * K + j];
            dst[j] = (uint8_t)b;
            acc |= (unsigned long long)b << have;
            have += 8;
            if (have >= kLdpcZ) { w[nw++] = (unsigned)acc & ((1u << kLdpcZ) - 1u); acc >>= kLdpcZ; have -= kLdpcZ; }
        }
        static_assert((8 * K) / kLdpcZ == C::info_cols - 1, "the last info word is the partial one");
        w[C::info_cols - 1] = (unsigned)acc; // the last info bits; the shortened ones behind them are 0
        parity<RATE>(w, par, typename C::Rows{});
        acc = 0; have = 0;
        int o = K;
#pragma unroll
        for (int j = 0; j < C::rows; ++j) {
            acc |= (unsigned long long)par[j] << have;
            have += kLdpcZ;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (have >= 8 && o < kLdpcCodeBytes) { dst[o++] = (uint8_t)acc; acc >>= 8; have -= 8; }
        }
    }
}

namespace {
// waves per SIMD (= workgroups per CU) the decode kernels are sized for: see the resource table in DESIGN.md section 3
template <int RATE> constexpr long long decode_workgroups_per_cu() { return RATE == 0 ? 5 : 4; }

template <int RATE>
hipError_t launch_decode(const LdpcDecodeParams &p, int num_cu, const Tuning *tune, hipStream_t st) {
    const long long blocks = persistent_grid((p.n_frames + 3) / 4, decode_workgroups_per_cu<RATE>() * num_cu, tuning_or_default(tune));
    hipLaunchKernelGGL(k_ldpc_decode<RATE>, dim3((unsigned)blocks), dim3(256), 0, st, p);
    return hipGetLastError();
}
template <int RATE>
hipError_t launch_encode(const LdpcEncodeParams &p, long long units, int num_cu, const Tuning *tune, hipStream_t st) {
    const long long blocks = persistent_grid((units + 255) / 256, 8LL * num_cu, tuning_or_default(tune));
    hipLaunchKernelGGL(k_ldpc_encode<RATE>, dim3((unsigned)blocks), dim3(256), 0, st, p);
    return hipGetLastError();
}
} // namespace

const char *ldpc_decode_name(int rate) {
    static const char *const names[] = {"k_ldpc_decode", "k_ldpc_decode<r23>", "k_ldpc_decode<r34>", "k_ldpc_decode<r56>"};
    return rate >= 0 && rate < kLdpcRates ? names[rate] : "";
}
const char *ldpc_encode_name(int rate) {
    static const char *const names[] = {"k_ldpc_encode", "k_ldpc_encode<r23>", "k_ldpc_encode<r34>", "k_ldpc_encode<r56>"};
    return rate >= 0 && rate < kLdpcRates ? names[rate] : "";
}

// any rate outside 0 .. 3 is an error (no kernel is no result)
hipError_t run_ldpc_decode(const LdpcDecodeParams &p, int rate, int num_cu, const Tuning *tune, hipStream_t st) {
    if (p.n_frames <= 0) return hipSuccess;
    switch (rate) {
    case 0: return launch_decode<0>(p, num_cu, tune, st);
    case 1: return launch_decode<1>(p, num_cu, tune, st);
    case 2: return launch_decode<2>(p, num_cu, tune, st);
    case 3: return launch_decode<3>(p, num_cu, tune, st);
    }
    return hipErrorInvalidValue;
}
hipError_t run_ldpc_encode(const LdpcEncodeParams &p, int rate, int num_cu, const Tuning *tune, hipStream_t st) {
    const long long units = p.n_frames * p.n_cw;
    if (units <= 0) return hipSuccess;
    switch (rate) {
    case 0: return launch_encode<0>(p, units, num_cu, tune, st);
    case 1: return launch_encode<1>(p, units, num_cu, tune, st);
    case 2: return launch_encode<2>(p, units, num_cu, tune, st);
    case 3: return launch_encode<3>(p, units, num_cu, tune, st);
    }
    return hipErrorInvalidValue;
}

} // namespace ofdm
