// kernels_fcs.hip -- the CRC-32 frame check (ofdm_fcs_wrap_batch / ofdm_fcs_check_batch and the frame modes ecc = OFDM_ECC_FCS + mode;
// include/ofdm_hip.h "frame check sequence", DESIGN.md section 3, definition: tests/fcs_ref.py over zlib.crc32).
//   crc32 = IEEE 802.3: reflected polynomial 0xEDB88320, register 0xFFFFFFFF at the start, result complemented.
//   envelope of p payload bytes = [u32 LE p] ++ payload ++ [u32 LE crc32 of the p + 4 bytes in front of it].
// One wavefront per row on a persistent grid, both kernels over one routine, wave_crc32:
//   * the message (m = p + 4 bytes) is aligned at its END: with the launch-uniform chunk c (a multiple of 4, 64 c >= the longest
//     message of the launch) lane l owns message bytes [m - (64 - l) c, m - (63 - l) c); indices below 0 are zero bytes.
//   * crc0 = the CRC with a zero register and no final complement is linear: leading zero bytes do not change it, and
//     crc32(msg) = ~crc0(msg with its first four bytes complemented).  Every lane reduces its chunk to crc0 on its own (slice-by-4
//     through four 1 KB tables in LDS; bit-serial in registers behind the laboratory key fcs_bitserial).
//   * crc0(A ++ B) = crc0(A) x^(8 |B|) mod P xor crc0(B): six levels, level k multiplies by the wave-uniform x^(8 c 2^k) mod P -- the
//     multiplier's x^i multiples stay in scalar registers, the lane's value selects among them, 32 conditional xors -- and takes the
//     neighbour 2^k lanes below.  Lane 63 ends with the whole message's crc0.  The six constants come from the host.
// The reducing pass is also the copying pass (Sink): message byte i is envelope byte i (wrap) and payload byte i - 4 (check).
// Every read of k_fcs_check stays inside [row, row + L_f): the length word is compared with L_f - 8 before anything is read by it.
#include "device_common.hpp"
#include "kernels.hpp"

namespace ofdm {

namespace {
constexpr unsigned kCrcPoly = 0xEDB88320u;

__host__ __device__ inline unsigned crc_times_x(unsigned v) { return (v >> 1) ^ ((v & 1u) ? kCrcPoly : 0u); }

// a(x) b(x) mod P in the reflected representation (bit 31 = x^0); host side
inline unsigned crc_mulmod_host(unsigned a, unsigned b) {
    unsigned p = 0;
    for (int i = 31; i >= 0; --i) { if ((a >> i) & 1u) p ^= b; b = crc_times_x(b); }
    return p;
}

// v(x) k(x) mod P, k the same in every lane: its multiples k x^i are scalar values
__device__ __forceinline__ unsigned crc_mulmod_uniform(unsigned v, unsigned k) {
    unsigned p = 0;
#pragma unroll
    for (int i = 31; i >= 0; --i) {
        p ^= (unsigned)(-(int)((v >> i) & 1u)) & k;
        k = crc_times_x(k);
    }
    return p;
}

// T[0][i] = the byte table, T[k][i] = T[0][i] advanced by k zero bytes: 256 threads
__device__ __forceinline__ void crc_load_tables(unsigned (*T)[256], int tid) {
    unsigned v = (unsigned)tid;
#pragma unroll
    for (int b = 0; b < 8; ++b) v = crc_times_x(v);
    T[0][tid] = v;
    __syncthreads();
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        v = (v >> 8) ^ T[0][v & 0xFFu];
        T[k][tid] = v;
    }
    __syncthreads();
}

template <bool kBits> __device__ __forceinline__ unsigned crc_dword(unsigned crc, unsigned w, const unsigned (*T)[256]) {
    crc ^= w;
    if (kBits) {
#pragma unroll
        for (int b = 0; b < 32; ++b) crc = crc_times_x(crc);
        return crc;
    }
    return T[3][crc & 0xFFu] ^ T[2][(crc >> 8) & 0xFFu] ^ T[1][(crc >> 16) & 0xFFu] ^ T[0][crc >> 24];
}

// crc32 of the m >= 4 message bytes src.get(0 .. m - 1), the same value in every lane; sink.put(i, byte) sees every message byte once.
// 64 c >= m, c a multiple of 4; K[k] = x^(8 c 2^k) mod P.
template <bool kBits, class Src, class Sink>
__device__ __forceinline__ unsigned wave_crc32(const Src &src, const Sink &sink, long long m, int c, const unsigned (&K)[6], int lane,
                                                const unsigned (*T)[256]) {
    const long long first = m - (long long)(64 - lane) * c;
    unsigned crc = 0;
    for (int j = 0; j < c; j += 4) {
        const long long i0 = first + j;
        if (i0 + 3 < 0) continue; // zero bytes in front of the message leave a zero register as it is
        unsigned w = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const long long i = i0 + b;
            if (i >= 0) {
                const unsigned v = src.get(i);
                sink.put(i, (uint8_t)v);
                w |= (i < 4 ? v ^ 0xFFu : v) << (8 * b);
            }
        }
        crc = crc_dword<kBits>(crc, w, T);
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) { // lanes whose low k + 1 bits are ones hold the crc0 of their 2^(k + 1) chunks
        const unsigned t = crc_mulmod_uniform(crc, K[k]);
        crc ^= (unsigned)__shfl_xor((int)t, 1 << k, 64);
    }
    return ~(unsigned)__builtin_amdgcn_readlane((int)crc, 63);
}

struct WrapSrc { // [u32 LE p] ++ payload
    const uint8_t *in;
    unsigned p;
    __device__ __forceinline__ unsigned get(long long i) const { return i < 4 ? (p >> (8 * (int)i)) & 0xFFu : (unsigned)in[i - 4]; }
};
struct WrapSink { // message byte i = envelope byte i
    uint8_t *out;
    __device__ __forceinline__ void put(long long i, uint8_t v) const { out[i] = v; }
};
struct CheckSrc {
    const uint8_t *row;
    __device__ __forceinline__ unsigned get(long long i) const { return row[i]; }
};
struct CheckSink { // message byte i >= 4 = payload byte i - 4
    uint8_t *out;
    __device__ __forceinline__ void put(long long i, uint8_t v) const { if (i >= 4) out[i - 4] = v; }
};

__device__ __forceinline__ long long row_len(const int32_t *len, long long f, long long n) {
    if (!len) return n;
    const long long v = len[f];
    return v < 0 ? 0 : (v > n ? n : v);
}
} // namespace

// Row f: len_f payload bytes (in_len[f] clamped to [0, n_bytes], or n_bytes) -> the envelope of len_f + 8 bytes, zeros behind it up
// to n_bytes + 8; out_len[f] (optional) = len_f + 8.
template <bool kBits> __global__ __launch_bounds__(256) void k_fcs_wrap(FcsWrapParams p) {
    __shared__ unsigned T[4][256];
    if (!kBits) crc_load_tables(T, threadIdx.x);
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (long long)gridDim.x * 4;
    for (long long f = wave; f < p.n_frames; f += n_waves) {
        const long long len = row_len(p.in_len, f, p.n_bytes);
        uint8_t *dst = p.out + f * p.out_stride;
        const WrapSrc src{p.in + f * p.in_stride, (unsigned)len};
        const unsigned crc = wave_crc32<kBits>(src, WrapSink{dst}, len + 4, p.chunk, p.K, lane, T);
        for (long long i = len + 4 + lane; i < p.n_bytes + 8; i += 64) dst[i] = i < len + 8 ? (uint8_t)(crc >> (8 * (int)(i - len - 4))) : (uint8_t)0;
        if (lane == 0 && p.out_len) p.out_len[f] = (int32_t)(len + 8);
    }
}

// Row f: L_f bytes (row_len[f] clamped to [0, n_row], or n_row).  Valid iff L_f >= 8, p = the u32 at byte 0 <= L_f - 8 and the u32 at
// byte 4 + p is crc32(row[0 : 4 + p]); then the payload is at out + f out_stride, out_len[f] = p, ok[f] = 1; else out_len[f] = 0,
// ok[f] = 0 (the row at out may hold bytes of the rejected payload).  Chain mode (status_rw != nullptr; row_len and out_len may be the
// same array): a row whose status is not 0 is skipped with out_len 0; an invalid one gets status OFDM_FRAME_FCS.
template <bool kBits> __global__ __launch_bounds__(256) void k_fcs_check(FcsCheckParams p) {
    __shared__ unsigned T[4][256];
    if (!kBits) crc_load_tables(T, threadIdx.x);
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (long long)gridDim.x * 4;
    for (long long f = wave; f < p.n_frames; f += n_waves) {
        if (p.status_rw && p.status_rw[f] != 0) { if (lane == 0) p.out_len[f] = 0; continue; }
        const long long L = row_len(p.row_len, f, p.n_row);
        const uint8_t *row = p.row + f * p.row_stride;
        bool valid = L >= 8;
        long long plen = 0;
        if (valid) {
            plen = (long long)((unsigned)row[0] | (unsigned)row[1] << 8 | (unsigned)row[2] << 16 | (unsigned)row[3] << 24);
            valid = plen <= L - 8; // (64 bits: a length word of 0xFFFFFFFF is a large number, not -1)
        }
        if (valid) {
            const unsigned crc = wave_crc32<kBits>(CheckSrc{row}, CheckSink{p.out + f * p.out_stride}, plen + 4, p.chunk, p.K, lane, T);
            const uint8_t *fcs = row + 4 + plen; // inside the row: 4 + plen + 4 <= L
            valid = crc == ((unsigned)fcs[0] | (unsigned)fcs[1] << 8 | (unsigned)fcs[2] << 16 | (unsigned)fcs[3] << 24);
        }
        if (lane == 0) {
            if (p.out_len) p.out_len[f] = valid ? (int32_t)plen : 0;
            if (p.ok) p.ok[f] = valid ? 1 : 0;
            if (p.status_rw && !valid) p.status_rw[f] = -6; // OFDM_FRAME_FCS
        }
    }
}

uint32_t crc32_host(const uint8_t *data, long long n) {
    static const struct Tab {
        unsigned t[4][256];
        Tab() {
            for (unsigned i = 0; i < 256; i++) { unsigned v = i; for (int b = 0; b < 8; b++) v = crc_times_x(v); t[0][i] = v; }
            for (int k = 1; k < 4; k++) for (unsigned i = 0; i < 256; i++) t[k][i] = (t[k - 1][i] >> 8) ^ t[0][t[k - 1][i] & 0xFFu];
        }
    } tab;
    unsigned crc = 0xFFFFFFFFu;
    long long i = 0;
    for (; i + 4 <= n; i += 4) { // bytes, not a dword load: any alignment, any endianness
        crc ^= (unsigned)data[i] | (unsigned)data[i + 1] << 8 | (unsigned)data[i + 2] << 16 | (unsigned)data[i + 3] << 24;
        crc = tab.t[3][crc & 0xFFu] ^ tab.t[2][(crc >> 8) & 0xFFu] ^ tab.t[1][(crc >> 16) & 0xFFu] ^ tab.t[0][crc >> 24];
    }
    for (; i < n; i++) crc = (crc >> 8) ^ tab.t[0][(crc ^ data[i]) & 0xFFu];
    return ~crc;
}

// chunk and combine constants of a launch whose longest message is max_msg bytes
static void fcs_plan(long long max_msg, int &chunk, unsigned (&K)[6]) {
    const long long q = max_msg > 0 ? (max_msg + 255) / 256 : 1;
    chunk = (int)(4 * q); // max_msg <= 2^31 + 3: fits
    unsigned k = 0x80000000u; // x^0
    unsigned sq = crc_times_x(k); // x^1, squared up to x^(8 chunk) by the bits of the exponent
    for (long long e = 8LL * chunk; e; e >>= 1) { if (e & 1) k = crc_mulmod_host(k, sq); sq = crc_mulmod_host(sq, sq); }
    for (int i = 0; i < 6; i++) { K[i] = k; k = crc_mulmod_host(k, k); }
}

// Persistent grids of 256 threads (four rows in flight a workgroup), seven workgroups per CU: 106 SGPRs (the multiples of the combine
// constants) allow seven wavefronts per SIMD; 35 - 68 VGPRs and 4 KB of LDS would allow more
hipError_t run_fcs_wrap(FcsWrapParams p, int num_cu, const Tuning *tune, hipStream_t st) {
    if (p.n_frames <= 0) return hipSuccess;
    const Tuning &tu = tuning_or_default(tune);
    fcs_plan(p.n_bytes + 4, p.chunk, p.K);
    const long long blocks = persistent_grid((p.n_frames + 3) / 4, 7LL * num_cu, tu);
    if (tu.fcs_bitserial) hipLaunchKernelGGL(k_fcs_wrap<true>, dim3((unsigned)blocks), dim3(256), 0, st, p);
    else hipLaunchKernelGGL(k_fcs_wrap<false>, dim3((unsigned)blocks), dim3(256), 0, st, p);
    return hipGetLastError();
}
hipError_t run_fcs_check(FcsCheckParams p, int num_cu, const Tuning *tune, hipStream_t st) {
    if (p.n_frames <= 0) return hipSuccess;
    const Tuning &tu = tuning_or_default(tune);
    fcs_plan(p.n_row - 4, p.chunk, p.K);
    const long long blocks = persistent_grid((p.n_frames + 3) / 4, 7LL * num_cu, tu);
    if (tu.fcs_bitserial) hipLaunchKernelGGL(k_fcs_check<true>, dim3((unsigned)blocks), dim3(256), 0, st, p);
    else hipLaunchKernelGGL(k_fcs_check<false>, dim3((unsigned)blocks), dim3(256), 0, st, p);
    return hipGetLastError();
}

} // namespace ofdm
