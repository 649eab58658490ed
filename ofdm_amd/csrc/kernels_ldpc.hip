// kernels_ldpc.hip -- the LDPC(648,324) code of OFDM_ECC_LDPC648 on the device (ofdm_ldpc648_encode_batch / _decode_batch and the
// mode's frame chain; include/ofdm_hip.h "LDPC(648,324)").  The code and the decoding rule are those of
// ldpc_table.h / ldpc_code.hip / tests/ldpc_ref.py, which the kernels are held to bit for bit, iteration counts included.
//   k_ldpc_decode  one wavefront per frame, four to a workgroup, persistent grid.  The wavefront takes its frame's code words two at
//                  a time: lanes 0 .. 26 and 32 .. 58, lane = check z of ALL twelve block rows.  The 648 posteriors Q of a code word
//                  sit in a slab of LDS owned by the half-wavefront (int16; the two slabs 32 banks apart), so a block row reads and
//                  writes 27 consecutive int16 per block apart from the wrap, and nothing needs a barrier: one wavefront's LDS
//                  accesses are ordered.  The 88 check messages R_e of a lane are not stored one by one: after a row's update every
//                  R_e is sign_e times one of TWO magnitudes (min((3 m) >> 2, 127) of the smallest |T| for every edge but the one
//                  that holds it, of the second smallest for that one), so a row keeps both magnitudes, the position of the smallest
//                  and its sign bits in ONE dword -- twelve VGPRs instead of 88, the same integers.
//                  After an iteration lane z reads Q[27 c + z] for the 24 block columns; one ballot a column gives both halves'
//                  27-bit words of hard decisions in scalar registers, and the 324 checks are 88 rotate-xors on them in scalar code.
//                  A converged half is masked off while the other goes on.  The frame's verdict, length and status are wave-uniform:
//                  lane 0 writes them, no atomics, no second launch.
//   k_ldpc_encode  one thread per code word: the twelve 27-bit info words, lambda_l by rotate-xor, back-substitution along the dual
//                  diagonal (ldpc_table.h).  Chain mode builds the info stream [u32 LE p][u32 LE ~p] ++ payload on the fly.
#include "device_common.hpp"
#include "kernels.hpp"
#include "ldpc_table.h"

#include <utility>

namespace ofdm {

namespace {
constexpr int kLdpcSlab = 704; // int16 between the two slabs of a wavefront: 648 rounded up to 352 dwords = 32 banks (mod 64) apart

template <int E> struct LdpcEdge {
    static constexpr int col = kLdpcEdgeList.col[E], shift = kLdpcEdgeList.shift[E];
    // variable index of check z
    __device__ __forceinline__ static int var(int z) {
        if (shift == 0) return kLdpcZ * col + z;
        const int t = z + shift;
        return kLdpcZ * col + (t >= kLdpcZ ? t - kLdpcZ : t);
    }
};
template <int L> struct LdpcRow {
    static constexpr int first = kLdpcEdgeList.first[L], degree = kLdpcEdgeList.first[L + 1] - kLdpcEdgeList.first[L];
    static_assert(degree >= 2 && degree <= 8, "a row's state is packed for at most eight edges");
    using Edges = std::make_integer_sequence<int, degree>;
};

__device__ __forceinline__ void ldpc_wave_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }
__device__ __forceinline__ int ldpc_clamp(int v) { return v > kLdpcQMax ? kLdpcQMax : (v < -kLdpcQMax ? -kLdpcQMax : v); }
__device__ __forceinline__ int ldpc_scale(int m) { const int r = (3 * m) >> 2; return r > kLdpcRMax ? kLdpcRMax : r; }

// One block row for check z.  st = the row's messages: bits 0 .. 6 the magnitude of every edge but one, 7 .. 13 the magnitude of
// edge `bits 14 .. 16`, bit 17 + i the sign of edge i (1 = negative); 0 = every R is 0.
template <int L, int... I>
__device__ __forceinline__ void ldpc_row_update(int16_t *Q, int z, unsigned &st, std::integer_sequence<int, I...>) {
    constexpr int e0 = LdpcRow<L>::first, deg = sizeof...(I);
    const int a1 = (int)(st & 127u), a2 = (int)((st >> 7) & 127u), at = (int)((st >> 14) & 7u);
    int var[deg], T[deg];
    ((var[I] = LdpcEdge<e0 + I>::var(z)), ...);
    ((T[I] = ldpc_clamp((int)Q[var[I]] - (((st >> (17 + I)) & 1u) ? -(I == at ? a2 : a1) : (I == at ? a2 : a1)))), ...);
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
    const int n1 = ldpc_scale(m1), n2 = ldpc_scale(m2);
    const unsigned flip = (__popc(neg) & 1) ? (1u << deg) - 1u : 0u;
    const unsigned sgn = neg ^ flip; // sign_e = the product over the OTHER edges
    ((Q[var[I]] = (int16_t)ldpc_clamp(T[I] + (((sgn >> I) & 1u) ? -(I == where ? n2 : n1) : (I == where ? n2 : n1)))), ...);
    st = (unsigned)n1 | ((unsigned)n2 << 7) | ((unsigned)where << 14) | (sgn << 17);
}
template <int... L>
__device__ __forceinline__ void ldpc_iteration(int16_t *Q, int z, unsigned (&st)[kLdpcRows], std::integer_sequence<int, L...>) {
    ((ldpc_row_update<L>(Q, z, st[L], typename LdpcRow<L>::Edges{}), ldpc_wave_fence()), ...);
}

// bit z = the parity of check z of block row L over the hard-decision words w[c] of the block columns
template <int L, int... I>
__device__ __forceinline__ unsigned ldpc_row_syndrome(const unsigned (&w)[kLdpcCols], std::integer_sequence<int, I...>) {
    constexpr int e0 = LdpcRow<L>::first;
    return (ldpc_rot(w[LdpcEdge<e0 + I>::col], LdpcEdge<e0 + I>::shift) ^ ...);
}
template <int... L>
__device__ __forceinline__ unsigned ldpc_syndrome(const unsigned (&w)[kLdpcCols], std::integer_sequence<int, L...>) {
    return (ldpc_row_syndrome<L>(w, typename LdpcRow<L>::Edges{}) | ...);
}
using LdpcRows = std::make_integer_sequence<int, kLdpcRows>;

// the posteriors a code word starts from (ldpc_code.hip), all 64 lanes
__device__ __forceinline__ void ldpc_load(const int8_t *llr, int16_t *Q, int lane) {
#pragma unroll
    for (int v0 = 0; v0 < kLdpcN; v0 += 64) {
        const int v = v0 + lane;
        if (v < kLdpcN) {
            const bool sent = v < kLdpcInfoBits || (v >= kLdpcChecks && v < kLdpcChecks + kLdpcInfoBits);
            const int l = sent ? (int)llr[v < kLdpcInfoBits ? v : v - 4] : 0;
            Q[v] = (int16_t)(sent ? -l : (v < kLdpcChecks ? kLdpcQMax : 0));
        }
    }
}

struct LdpcPair {
    int it_a, it_b;        // the iteration at which each code word converged, 0 = not (wave-uniform)
    unsigned byte_a, byte_b; // lane i < 40: info byte i of each
};
// Decodes code word A (640 LLRs at llr_a) and, if llr_b is not null, code word B beside it.  slab: the wavefront's 2 * kLdpcSlab int16.
__device__ __forceinline__ LdpcPair ldpc_decode_pair(const int8_t *llr_a, const int8_t *llr_b, int max_iter, int16_t *slab, int lane) {
    const bool have_b = llr_b != nullptr; // (wave-uniform)
    ldpc_load(llr_a, slab, lane);
    if (have_b) ldpc_load(llr_b, slab + kLdpcSlab, lane);
    ldpc_wave_fence();
    const int z = lane & 31;
    const bool upper = lane >= 32, check = z < kLdpcZ;
    int16_t *Q = slab + (upper ? kLdpcSlab : 0);
    unsigned st[kLdpcRows];
#pragma unroll
    for (int l = 0; l < kLdpcRows; ++l) st[l] = 0;
    bool done_a = false, done_b = !have_b;
    LdpcPair r;
    r.it_a = 0; r.it_b = 0;
    for (int it = 1; it <= max_iter; ++it) {
        if (check && !(upper ? done_b : done_a)) ldpc_iteration(Q, z, st, LdpcRows{});
        ldpc_wave_fence();
        unsigned wa[kLdpcCols], wb[kLdpcCols];
#pragma unroll
        for (int c = 0; c < kLdpcCols; ++c) {
            const int q = check ? (int)Q[kLdpcZ * c + z] : 0;
            const unsigned long long b = __ballot(q < 0);
            wa[c] = (unsigned)b;
            wb[c] = (unsigned)(b >> 32);
        }
        if (!done_a && ldpc_syndrome(wa, LdpcRows{}) == 0) { done_a = true; r.it_a = it; }
        if (!done_b && ldpc_syndrome(wb, LdpcRows{}) == 0) { done_b = true; r.it_b = it; }
        if (done_a && done_b) break;
    }
    r.byte_a = 0; r.byte_b = 0;
    if (lane < kLdpcInfoBytes) {
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            r.byte_a |= (slab[8 * lane + b] < 0 ? 1u : 0u) << b;
            r.byte_b |= (slab[kLdpcSlab + 8 * lane + b] < 0 ? 1u : 0u) << b;
        }
    }
    ldpc_wave_fence(); // the next pair's load overwrites the slabs
    return r;
}
__device__ __forceinline__ unsigned ldpc_word_le(unsigned bytes, int first) { // the u32 in lanes first .. first + 3
    unsigned w = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) w |= ((unsigned)__builtin_amdgcn_readlane((int)bytes, first + i) & 0xFFu) << (8 * i);
    return w;
}
} // namespace

// Stage mode (status_rw == nullptr): row f holds n_cw code words of 640 LLRs; 40 n_cw bytes out, iters[f * n_cw + k] (optional).
// Chain mode (the frame mode): body = the demodulated bytes behind the 16-byte header (not read), nb = body / 80 whole code words
// from LLR 128 on.  nb = 0, code word 0 unconverged or its bytes 4 .. 7 not the complement of bytes 0 .. 3: status OFDM_FRAME_HEADER.
// Else with p = bytes 0 .. 3 and B = ceil((p + 8) / 40) the code words 1 .. min(B, nb) - 1 are decoded; one unconverged: status
// OFDM_FRAME_UNCORRECTABLE; else min(p, 40 nb - 8) bytes of the stream behind the two length words are delivered.
__global__ __launch_bounds__(256) void k_ldpc_decode(LdpcDecodeParams p) {
    __shared__ __attribute__((aligned(16))) int16_t q_lds[4][2 * kLdpcSlab];
    const int lane = threadIdx.x & 63;
    int16_t *slab = q_lds[threadIdx.x >> 6];
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (long long)gridDim.x * 4;
    for (long long f = wave; f < p.n_frames; f += n_waves) {
        const int8_t *l = p.llr + f * p.llr_stride;
        uint8_t *dst = p.out + f * p.out_stride;
        if (!p.status_rw) {
            for (long long k = 0; k < p.n_cw; k += 2) {
                const bool two = k + 1 < p.n_cw;
                const LdpcPair r = ldpc_decode_pair(l + k * kLdpcSentBits, two ? l + (k + 1) * kLdpcSentBits : nullptr, p.max_iter, slab, lane);
                if (lane < kLdpcInfoBytes) {
                    dst[k * kLdpcInfoBytes + lane] = (uint8_t)r.byte_a;
                    if (two) dst[(k + 1) * kLdpcInfoBytes + lane] = (uint8_t)r.byte_b;
                }
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
            const LdpcPair h = ldpc_decode_pair(l, nb >= 2 ? l + kLdpcSentBits : nullptr, p.max_iter, slab, lane);
            const unsigned len = ldpc_word_le(h.byte_a, 0), inv = ldpc_word_le(h.byte_a, 4);
            if (h.it_a == 0 || inv != ~len) status = -4;
            else {
                const long long want = (long long)(((unsigned long long)len + 8u + kLdpcInfoBytes - 1) / kLdpcInfoBytes);
                const long long n_cw = want < nb ? want : nb;
                bool bad = n_cw >= 2 && h.it_b == 0;
                if (!bad && lane < kLdpcInfoBytes) {
                    if (lane >= 8) dst[lane - 8] = (uint8_t)h.byte_a;
                    if (n_cw >= 2) dst[kLdpcInfoBytes - 8 + lane] = (uint8_t)h.byte_b;
                }
                for (long long k = 2; k < n_cw && !bad; k += 2) {
                    const bool two = k + 1 < n_cw;
                    const LdpcPair r = ldpc_decode_pair(l + k * kLdpcSentBits, two ? l + (k + 1) * kLdpcSentBits : nullptr, p.max_iter, slab, lane);
                    bad = r.it_a == 0 || (two && r.it_b == 0);
                    if (!bad && lane < kLdpcInfoBytes) {
                        dst[k * kLdpcInfoBytes - 8 + lane] = (uint8_t)r.byte_a;
                        if (two) dst[(k + 1) * kLdpcInfoBytes - 8 + lane] = (uint8_t)r.byte_b;
                    }
                }
                const long long room = kLdpcInfoBytes * nb - 8;
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
template <int L, int... C>
__device__ __forceinline__ unsigned ldpc_lambda(const unsigned (&u)[kLdpcRows], std::integer_sequence<int, C...>) {
    return ((kLdpcShift[L][C] >= 0 ? ldpc_rot(u[C], kLdpcShift[L][C] >= 0 ? kLdpcShift[L][C] : 0) : 0u) ^ ...);
}
template <int... L>
__device__ __forceinline__ void ldpc_parity(const unsigned (&u)[kLdpcRows], unsigned (&par)[kLdpcRows], std::integer_sequence<int, L...>) {
    unsigned lam[kLdpcRows];
    ((lam[L] = ldpc_lambda<L>(u, LdpcRows{})), ...);
    const unsigned p0 = (lam[L] ^ ...);
    par[0] = p0;
    ((L + 1 < kLdpcRows
          ? (void)(par[L + 1 < kLdpcRows ? L + 1 : 0] =
                       lam[L] ^ (L ? par[L] : 0u) ^ (kLdpcShift[L][kLdpcRows] >= 0 ? ldpc_rot(p0, kLdpcShift[L][kLdpcRows] >= 0 ? kLdpcShift[L][kLdpcRows] : 0) : 0u))
          : (void)0),
     ...);
}
} // namespace

// One code word per thread.  Stage mode (framed == 0): row f = n_cw blocks of 40 info bytes -> n_cw blocks of 80 code bytes.
// Chain mode: row f = len_f payload bytes (in_len[f] clamped to [0, n_bytes], or n_bytes) -> the code of the info stream [u32 LE
// len_f][u32 LE ~len_f] ++ payload, zero-padded to ceil((len_f + 8) / 40) code words; the code words behind them, up to n_cw, are
// written as zeros; out_len[f] (optional) = 80 ceil((len_f + 8) / 40).
__global__ __launch_bounds__(256) void k_ldpc_encode(LdpcEncodeParams p) {
    const long long units = p.n_frames * p.n_cw;
    for (long long u = (long long)blockIdx.x * 256 + threadIdx.x; u < units; u += (long long)gridDim.x * 256) {
        const long long f = u / p.n_cw, k = u - f * p.n_cw;
        const uint8_t *src = p.in + f * p.in_stride;
        uint8_t *dst = p.out + f * p.out_stride + k * kLdpcCodeBytes;
        long long len = p.n_bytes;
        if (p.framed) {
            if (p.in_len) { const long long v = p.in_len[f]; len = v < 0 ? 0 : (v > p.n_bytes ? p.n_bytes : v); }
            const long long own = ldpc_stream_codewords(len);
            if (k == 0 && p.out_len) p.out_len[f] = (int32_t)(kLdpcCodeBytes * own);
            if (k >= own) {
                for (int i = 0; i < kLdpcCodeBytes; ++i) dst[i] = 0;
                continue;
            }
        }
        unsigned w[kLdpcRows], par[kLdpcRows];
        unsigned long long acc = 0;
        int have = 0, nw = 0;
#pragma unroll
        for (int j = 0; j < kLdpcInfoBytes; ++j) {
            unsigned b;
            if (p.framed) {
                const long long i = k * kLdpcInfoBytes + j;
                const unsigned word = i < 4 ? (unsigned)len : ~(unsigned)len;
                b = i < 8 ? (word >> (8 * (i & 3))) & 0xFFu : (i - 8 < len ? (unsigned)src[i - 8] : 0u);
            } else b = src[k * kLdpcInfoBytes + j];
            dst[j] = (uint8_t)b;
            acc |= (unsigned long long)b << have;
            have += 8;
            if (have >= kLdpcZ) { w[nw++] = (unsigned)acc & ((1u << kLdpcZ) - 1u); acc >>= kLdpcZ; have -= kLdpcZ; }
        }
        w[kLdpcRows - 1] = (unsigned)acc; // the last 23 info bits; x[320 .. 323] = 0
        ldpc_parity(w, par, LdpcRows{});
        acc = 0; have = 0;
        int o = kLdpcInfoBytes;
#pragma unroll
        for (int j = 0; j < kLdpcRows; ++j) {
            acc |= (unsigned long long)par[j] << have;
            have += kLdpcZ;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (have >= 8 && o < kLdpcCodeBytes) { dst[o++] = (uint8_t)acc; acc >>= 8; have -= 8; }
        }
    }
}

// k_ldpc_decode: 88 VGPRs, four wavefronts and 11 KiB of LDS a workgroup: five workgroups per CU (five wavefronts per SIMD)
hipError_t run_ldpc_decode(const LdpcDecodeParams &p, int num_cu, const Tuning *tune, hipStream_t st) {
    if (p.n_frames <= 0) return hipSuccess;
    const long long blocks = persistent_grid((p.n_frames + 3) / 4, 5LL * num_cu, tuning_or_default(tune));
    hipLaunchKernelGGL(k_ldpc_decode, dim3((unsigned)blocks), dim3(256), 0, st, p);
    return hipGetLastError();
}
hipError_t run_ldpc_encode(const LdpcEncodeParams &p, int num_cu, const Tuning *tune, hipStream_t st) {
    const long long units = p.n_frames * p.n_cw;
    if (units <= 0) return hipSuccess;
    const long long blocks = persistent_grid((units + 255) / 256, 8LL * num_cu, tuning_or_default(tune));
    hipLaunchKernelGGL(k_ldpc_encode, dim3((unsigned)blocks), dim3(256), 0, st, p);
    return hipGetLastError();
}

} // namespace ofdm
