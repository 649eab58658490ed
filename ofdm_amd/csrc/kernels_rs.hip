// kernels_rs.hip -- the outer Reed-Solomon(255,223) code of the reference's demos (src/utils.rs:97-180) on the device, batched
// (ofdm_rs255_encode_batch / ofdm_rs255_decode_batch and the OFDM_ECC_RS255* frame modes; include/ofdm_hip.h).
// The code is the one of outer_code.hip, whose encode_block / correct_block are the definition the kernels are held to byte for
// byte: GF(2^8) with polynomial 0x11d, generator prod_{i<32} (x - 2^i), 32 parity bytes behind the data.
//   k_rs255_encode  one half-wavefront per 255-byte block, lane = parity coefficient: the 223 data bytes are divided by the monic
//                   generator in an LFSR that lives in one VGPR (the feedback byte is broadcast, the register shifts one lane down).
//   k_rs255_decode  one wavefront per row, its blocks one after the other (the row's corrected count and its "any block failed" flag
//                   stay in wave-uniform registers: no atomics, no second pass).  Lane l holds the block's bytes l, l + 64, l + 128,
//                   l + 192 (coalesced byte loads).  The 32 syndromes come first: every lane forms its four bytes' share of each
//                   (c X^i by stepping the exponent, one table read per term), four syndromes to a dword, and eight xor butterflies
//                   over the wavefront leave all 32 in every lane.  A block whose syndromes are zero leaves at once with its 223
//                   bytes.  Only a dirty block runs Berlekamp-Massey (lane = coefficient of sigma, the discrepancy by one xor
//                   reduction a step), the Chien search (lane = position, four positions a lane), Forney at the lanes that found a
//                   root, and the syndromes again over the corrected bytes -- correct_block's final check, which makes the outcome
//                   "the code word within 16 byte errors if there is one, failure otherwise" and so a function of the input alone.
// GF multiplication goes through log / exp tables of 256 bytes each in LDS (64 dwords = one per bank: no bank conflicts).
#include "device_common.hpp"
#include "kernels.hpp"

namespace ofdm {

namespace {
constexpr int kRsN = 255, kRsK = 223, kRsPar = kRsN - kRsK;

struct RsTables {
    uint8_t exp[256], log[256];
    uint8_t gen_log[kRsPar]; // log of generator coefficient j + 1, highest degree first (the leading 1 left out)
    bool gen_nonzero;
};
constexpr RsTables make_rs_tables() {
    RsTables t{};
    int x = 1;
    for (int i = 0; i < 255; i++) { t.exp[i] = (uint8_t)x; t.log[x] = (uint8_t)i; x <<= 1; if (x & 0x100) x ^= 0x11d; }
    t.exp[255] = 1;
    t.log[0] = 0;
    uint8_t g[kRsPar + 1] = {1};
    for (int i = 0; i < kRsPar; i++) { // g *= (x - 2^i)
        uint8_t ng[kRsPar + 1] = {};
        for (int j = 0; j <= i; j++) {
            ng[j] ^= g[j];
            if (g[j]) ng[j + 1] ^= t.exp[(t.log[g[j]] + i) % 255];
        }
        for (int j = 0; j <= kRsPar; j++) g[j] = ng[j];
    }
    t.gen_nonzero = true;
    for (int j = 0; j < kRsPar; j++) { t.gen_log[j] = t.log[g[j + 1]]; if (!g[j + 1]) t.gen_nonzero = false; }
    return t;
}
constexpr RsTables kRsHostTab = make_rs_tables();
static_assert(kRsHostTab.gen_nonzero, "the encoder multiplies by the generator's coefficients through their logs");
__constant__ RsTables kRsTab = make_rs_tables();

// the tables in LDS: ex[i] = 2^i (i < 255), lg[v] = log2 v (v > 0)
struct RsGf {
    const uint8_t *ex, *lg;
    __device__ __forceinline__ static unsigned mod255(unsigned v) { return v >= 255u ? v - 255u : v; } // v < 510
    __device__ __forceinline__ unsigned mul(unsigned a, unsigned b) const { return (a && b) ? ex[mod255((unsigned)lg[a] + lg[b])] : 0u; }
    __device__ __forceinline__ unsigned div(unsigned a, unsigned b) const { return a ? ex[mod255((unsigned)lg[a] + 255u - lg[b])] : 0u; } // b != 0
};
__device__ __forceinline__ void rs_load_tables(uint8_t *ex, uint8_t *lg, int tid) { // 256 threads
    ex[tid] = kRsTab.exp[tid];
    lg[tid] = kRsTab.log[tid];
    __syncthreads();
}
__device__ __forceinline__ unsigned wave_xor(unsigned v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v ^= (unsigned)__shfl_xor((int)v, o, 64);
    return v;
}

// S_i = sum_j c_j X_j^i, X_j = 2^(254 - j), i < 32: byte i & 3 of P[i >> 2], the same in every lane.  Byte k of cw is byte
// lane + 64 k of the block (0 for the position 255 that does not exist).  The loop over k stays a loop: unrolled, the compiler
// keeps all 128 table reads in flight and the kernel drops to two wavefronts per SIMD.
__device__ __forceinline__ void rs_syndromes(const RsGf &gf, unsigned cw, int lane, unsigned (&P)[8]) {
#pragma unroll
    for (int q = 0; q < 8; ++q) P[q] = 0;
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        const int pos = lane + 64 * k;
        const unsigned ck = (cw >> (8 * k)) & 0xFFu;
        const bool nz = ck != 0;
        const unsigned e = pos < kRsN ? (unsigned)(254 - pos) : 0u;
        unsigned idx = gf.lg[ck];
#pragma unroll
        for (int i = 0; i < kRsPar; ++i) {
            const unsigned v = nz ? (unsigned)gf.ex[idx] : 0u;
            P[i >> 2] ^= v << (8 * (i & 3));
            idx = RsGf::mod255(idx + e);
        }
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) P[q] = wave_xor(P[q]);
}
__device__ __forceinline__ bool rs_all_zero(const unsigned (&P)[8]) {
    return (P[0] | P[1] | P[2] | P[3] | P[4] | P[5] | P[6] | P[7]) == 0;
}

// correct_block (outer_code.hip) of a block whose syndromes P are not all zero, step for step.  cw is corrected in place; the return
// value is the number of corrected bytes or -1 (cw is then in an undefined state: the caller keeps its own copy).  scr: 160 bytes of
// LDS owned by this wavefront.
__device__ __forceinline__ int rs_correct(const RsGf &gf, unsigned &cw, const unsigned (&P)[8], int lane, uint8_t *scr) {
    uint8_t *sy = scr, *sg = scr + 32, *sl = scr + 72, *om = scr + 112; // syndromes, sigma, log sigma, omega
    wave_fence();
    if (lane < kRsPar) sy[lane] = (uint8_t)(P[lane >> 2] >> (8 * (lane & 3)));
    wave_fence();
    // Berlekamp-Massey, sigma(x) lowest degree first: lane = coefficient (kRsPar + 2 of them, as the host's arrays)
    unsigned sigma = lane == 0, prev = sigma;
    int L = 0, m = 1;
    unsigned b = 1;
    for (int n = 0; n < kRsPar; ++n) {
        const int si = n - lane;
        unsigned term = 0;
        if (lane <= L && si >= 0) term = gf.mul(sigma, sy[si]);
        const unsigned d = (unsigned)__builtin_amdgcn_readfirstlane((int)wave_xor(term));
        if (d == 0) { ++m; continue; }
        const unsigned t = sigma;
        const unsigned coef = gf.div(d, b);
        const unsigned sh = (unsigned)__shfl((int)prev, (lane - m) & 63, 64);
        if (lane >= m && lane < kRsPar + 2) sigma ^= gf.mul(coef, sh);
        if (2 * L <= n) { L = n + 1 - L; prev = t; b = d; m = 1; } else ++m;
    }
    if (L > kRsPar / 2) return -1;
    if (lane < kRsPar + 2) { sg[lane] = (uint8_t)sigma; sl[lane] = gf.lg[sigma]; }
    wave_fence();
    // Chien search: an error at byte j <=> sigma(X^-1) = 0 with X = 2^(254 - j), log X^-1 = (j + 1) mod 255
    unsigned roots = 0; // bit k: position lane + 64 k is a root
    int nerr = 0;
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        const int pos = lane + 64 * k;
        const unsigned xinv = pos + 1 >= kRsN ? (unsigned)(pos + 1 - kRsN) : (unsigned)(pos + 1);
        unsigned v = 0, acc = 0; // acc = (xinv * i) mod 255
        for (int i = 0; i <= L; ++i) {
            if (sg[i]) v ^= gf.ex[RsGf::mod255(sl[i] + acc)];
            acc = RsGf::mod255(acc + xinv);
        }
        const bool root = pos < kRsN && v == 0;
        roots |= (root ? 1u : 0u) << k;
        nerr += __popcll(__ballot(root));
    }
    if (nerr != L) return -1;
    // Forney (first consecutive root 0): e = X Omega(X^-1) / sigma'(X^-1), Omega = S(x) sigma(x) mod x^32
    if (lane < kRsPar) {
        unsigned o = 0;
        for (int j = 0; j <= L && j <= lane; ++j) o ^= gf.mul(sg[j], sy[lane - j]);
        om[lane] = (uint8_t)o;
    }
    wave_fence();
    bool den_zero = false;
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        if ((roots >> k) & 1u) {
            const int pos = lane + 64 * k, lx = 254 - pos;
            const unsigned lxi = lx ? (unsigned)(255 - lx) : 0u;
            unsigned num = 0, den = 0, acc = 0; // acc = (lxi * i) mod 255
            for (int i = 0; i < kRsPar; ++i) {
                const unsigned o = om[i];
                if (o) num ^= gf.ex[RsGf::mod255(gf.lg[o] + acc)];
                // formal derivative: the odd-degree terms, sigma_{i+1} X^-i for even i
                if (!(i & 1) && i + 1 <= L && sg[i + 1]) den ^= gf.ex[RsGf::mod255(sl[i + 1] + acc)];
                acc = RsGf::mod255(acc + lxi);
            }
            if (den == 0) den_zero = true;
            else cw ^= gf.mul(gf.ex[lx], gf.div(num, den)) << (8 * k);
        }
    }
    if (__ballot(den_zero)) return -1;
    unsigned Q[8]; // a corrected block must be a code word
    rs_syndromes(gf, cw, lane, Q);
    return rs_all_zero(Q) ? nerr : -1;
}
} // namespace

// One row per wavefront.  Row f holds len_f code bytes (code_len[f] clamped to [0, n_code], or n_code) = len_f / 255 + 1 blocks, the
// last one zero-padded (and not computed at all when it is empty); 223 bytes leave per block, corrected where the block decodes, as
// received where it does not.  corrected[f] = corrected bytes of the row, -1 if a block failed.  Stage mode (status_rw == nullptr):
// out_len[f] = 223 (len_f / 255 + 1).  Chain mode: a row whose status is not 0 is skipped with out_len 0; a failed block makes the
// row's status OFDM_FRAME_UNCORRECTABLE and its out_len 0.  code_len and out_len may be the same array.
__global__ __launch_bounds__(256) void k_rs255_decode(Rs255DecodeParams p) {
    __shared__ uint8_t ex[256], lg[256];
    __shared__ uint8_t scratch[4][160];
    rs_load_tables(ex, lg, threadIdx.x);
    const RsGf gf{ex, lg};
    const int lane = threadIdx.x & 63;
    uint8_t *scr = scratch[threadIdx.x >> 6];
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (long long)gridDim.x * 4;
    for (long long f = wave; f < p.n_frames; f += n_waves) {
        if (p.status_rw && p.status_rw[f] != 0) { if (lane == 0) p.out_len[f] = 0; continue; }
        long long len = p.n_code;
        if (p.code_len) { const long long v = p.code_len[f]; len = v < 0 ? 0 : (v > p.n_code ? p.n_code : v); }
        const long long n_blocks = len / kRsN + 1;
        const uint8_t *src = p.code + f * p.code_stride;
        uint8_t *dst = p.out + f * p.out_stride;
        int total = 0;
        bool bad = false;
        for (long long b = 0; b < n_blocks; ++b) {
            const long long have = len - b * kRsN;
            unsigned cw = 0; // byte k = byte lane + 64 k of the block
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int pos = lane + 64 * k;
                if (pos < kRsN && pos < have) cw |= (unsigned)src[b * kRsN + pos] << (8 * k);
            }
            const unsigned rx = cw;
            if (have > 0) {
                unsigned P[8];
                rs_syndromes(gf, cw, lane, P);
                if (__builtin_amdgcn_readfirstlane((int)!rs_all_zero(P))) { // (the same in every lane)
                    const int r = __builtin_amdgcn_readfirstlane(rs_correct(gf, cw, P, lane, scr));
                    if (r < 0) { bad = true; cw = rx; } else total += r;
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int pos = lane + 64 * k;
                if (pos < kRsK) dst[b * kRsK + pos] = (uint8_t)(cw >> (8 * k));
            }
        }
        if (lane == 0) {
            if (p.corrected) p.corrected[f] = bad ? -1 : total;
            if (p.status_rw && bad) p.status_rw[f] = -5; // OFDM_FRAME_UNCORRECTABLE
            if (p.out_len) p.out_len[f] = (p.status_rw && bad) ? 0 : (int32_t)(kRsK * n_blocks);
        }
    }
}

// One block per half-wavefront.  Row f holds len_f data bytes (in_len[f] clamped to [0, n_bytes], or n_bytes) = len_f / 223 + 1
// blocks, the last one zero-padded; the blocks behind them, up to n_bytes / 223 + 1, are written as zeros.  An empty block's parity
// is zero as well.  Lane l of the half holds the data bytes l + 32 k and remainder coefficient l (highest degree in lane 0).
__global__ __launch_bounds__(256) void k_rs255_encode(Rs255EncodeParams p) {
    __shared__ uint8_t ex[256], lg[256];
    rs_load_tables(ex, lg, threadIdx.x);
    const int hl = threadIdx.x & 31;
    const unsigned lgen = kRsTab.gen_log[hl];
    const long long row_blocks = p.n_bytes / kRsK + 1, units = p.n_frames * row_blocks;
    for (long long u = (long long)blockIdx.x * 8 + (threadIdx.x >> 5); u < units; u += (long long)gridDim.x * 8) {
        const long long f = u / row_blocks, b = u - f * row_blocks;
        long long len = p.n_bytes;
        if (p.in_len) { const long long v = p.in_len[f]; len = v < 0 ? 0 : (v > p.n_bytes ? p.n_bytes : v); }
        uint8_t *dst = p.out + f * p.out_stride + b * kRsN;
        if (b == 0 && hl == 0 && p.out_len) p.out_len[f] = (int32_t)(kRsN * (len / kRsK + 1));
        const long long have = len - b * kRsK;
        if (have <= 0) {
            for (int i = hl; i < kRsN; i += 32) dst[i] = 0;
            continue;
        }
        const uint8_t *src = p.in + f * p.in_stride + b * kRsK;
        unsigned d[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const int pos = hl + 32 * k;
            d[k] = (pos < kRsK && pos < have) ? (unsigned)src[pos] : 0u;
            if (pos < kRsK) dst[pos] = (uint8_t)d[k];
        }
        unsigned rem = 0;
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            for (int j = 0; j < 32 && 32 * k + j < kRsK; ++j) { // synthetic division by the monic generator
                const unsigned fb = (unsigned)__shfl((int)d[k], j, 32) ^ (unsigned)__shfl((int)rem, 0, 32);
                unsigned nx = (unsigned)__shfl_down((int)rem, 1, 32);
                if (hl == 31) nx = 0;
                rem = nx ^ (fb ? (unsigned)ex[RsGf::mod255(lgen + lg[fb])] : 0u);
            }
        }
        dst[kRsK + hl] = (uint8_t)rem;
    }
}

// Persistent grids of 256 threads, five workgroups per CU: both kernels take about 90 VGPRs, five wavefronts per SIMD.
hipError_t run_rs255_encode(const Rs255EncodeParams &p, int num_cu, const Tuning *tune, hipStream_t st) {
    const long long units = p.n_frames * (p.n_bytes / kRsK + 1);
    if (units <= 0) return hipSuccess;
    const long long blocks = persistent_grid((units + 7) / 8, 5LL * num_cu, tuning_or_default(tune));
    hipLaunchKernelGGL(k_rs255_encode, dim3((unsigned)blocks), dim3(256), 0, st, p);
    return hipGetLastError();
}
hipError_t run_rs255_decode(const Rs255DecodeParams &p, int num_cu, const Tuning *tune, hipStream_t st) {
    if (p.n_frames <= 0) return hipSuccess;
    const long long blocks = persistent_grid((p.n_frames + 3) / 4, 5LL * num_cu, tuning_or_default(tune));
    hipLaunchKernelGGL(k_rs255_decode, dim3((unsigned)blocks), dim3(256), 0, st, p);
    return hipGetLastError();
}

} // namespace ofdm
