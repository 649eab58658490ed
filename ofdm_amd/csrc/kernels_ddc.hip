// kernels_ddc.hip -- EXT-16: the digital down-converter in front of a stream (ofdm_ddc_push, ofdm_stream_set_ddc; definition:
// include/ofdm_hip.h "a digital down-converter", numpy restatement: tests/ddc_ref.py).
//   k_ddc<fc32>   v[n] = x[n] (x) (C[p >> 10] (x) F[p & 1023]), p = (n phase_inc) mod 2^20;  y[m] = sum_k h[k] v[m D + k], ascending k, fmaf
//   k_ddc<sc16>   the same on x = (float)q * scale per component (sc16_widen1: the product is its own v_mul_f32)
// ONE launch per piece of a push converts the piece AND writes the carry the next piece reads.  n is the absolute sample index of the
// converter's stream: t0 samples lie in front of the piece, the last t0 - D M(t0) of them in the carry (raw, widened; at most T - 1).
// The units of the persistent grid, none of which reads what another writes:
//   tile   `tile` consecutive outputs (a multiple of kDdcR, at most 256 kDdcR, as many as the LDS image holds).  The workgroup mixes the
//          tile D + T - D input samples under the tile ONCE into LDS: a sample in front of the piece from the carry, one inside it with
//          16-byte loads (two fc32 or four sc16 samples; groups are aligned on `in`'s own 16-byte grid, so a base on 8 bytes only costs the
//          ragged ends, which go sample by sample).  Then thread t owns the kDdcR consecutive outputs t kDdcR ..: it walks the
//          (kDdcR - 1) D + T samples under them once, reads each from LDS once, and feeds it to every output whose window holds it --
//          output r takes sample j with tap k = j - r D, so every output's sum still runs in ascending k.  The taps are uniform over the
//          workgroup: they come through the scalar cache (constant address space), not through LDS or VGPRs.
//          LDS: sample s of the tile lies at s + s / (kDdcR D): one pad every thread's worth of samples, so that the threads of a
//          wavefront, kDdcR D samples apart, start on kDdcR D + 1 (odd) 8-byte words apart and a ds_read_b64 of the wavefront touches all
//          banks evenly for every D (a power of two times 8 bytes would put the whole wavefront on one or two banks).
//   carry  256 raw samples a unit of what lies behind the piece's last output, into the OTHER copy of the carry.
// The carry is double-buffered, so every unit reads the copy the previous launch wrote while this launch writes the other.  No atomics;
// nothing depends on the grid.
#include "device_common.hpp"
#include "kernels.hpp"

namespace ofdm {

constexpr int kDdcR = 4;      // consecutive outputs a thread keeps in registers
constexpr int kDdcLds = 6144; // float2 slots of the LDS image (48 KiB: three workgroups a CU)

struct DdcLaunch {
    DdcParams p;
    long long m0 = 0, m1 = 0; // outputs in front of the piece / behind it
    long long c0 = 0, c1 = 0; // the stream index of carry_old[0] / carry_new[0]
    long long tiles = 0, units = 0;
    int tile = 0;             // outputs per tile
    unsigned rd_magic = 0;    // ceil(2^32 / (kDdcR D)): s / (kDdcR D) = umulhi(s, rd_magic) for s < 2^13
    int mis = 0;              // samples by which `in` lies behind a 16-byte boundary
};

// one rounded f32 product that nothing can contract (HIP compiles with -ffp-contract=fast)
__device__ __forceinline__ float ddc_mul(float a, float b) {
    float y;
    asm("v_mul_f32 %0, %1, %2" : "=v"(y) : "v"(a), "v"(b));
    return y;
}
// a (x) b of the definition
__device__ __forceinline__ float2 ddc_cmul(float2 a, float2 b) {
    return make_float2(fmaf(a.x, b.x, -ddc_mul(a.y, b.y)), fmaf(a.x, b.y, ddc_mul(a.y, b.x)));
}
// sample i of the stream, mixed
__device__ __forceinline__ float2 ddc_mix(const DdcParams &p, float2 x, long long i) {
    const unsigned ph = ((unsigned)i * p.phase_inc) & (unsigned)kDdcPhaseMask; // 2^20 divides 2^32: the low words are enough
    return ddc_cmul(x, ddc_cmul(p.coarse[ph >> 10], p.fine[ph & 1023]));
}
// raw sample i of the stream, c0 <= i < t0 + n: out of the carry or out of the piece
template <bool SC16> __device__ __forceinline__ float2 ddc_raw(const DdcLaunch &a, long long i) {
    if (i < a.p.t0) return a.p.carry_old[i - a.c0];
    if constexpr (SC16) return sc16_widen1(static_cast<const uint32_t *>(a.p.in)[i - a.p.t0], a.p.scale);
    else return static_cast<const float2 *>(a.p.in)[i - a.p.t0];
}
__device__ __forceinline__ int ddc_pos(const DdcLaunch &a, int s) { return s + (int)__umulhi((unsigned)s, a.rd_magic); }

template <bool CHECK>
__device__ __forceinline__ void ddc_feed(float2 (&acc)[kDdcR], float2 v, const __attribute__((address_space(4))) float *h, int j, int D, int T) {
#pragma unroll
    for (int r = 0; r < kDdcR; ++r) {
        const int k = j - r * D;
        if (!CHECK || (k >= 0 && k < T)) {
            const float hk = h[k];
            acc[r].x = fmaf(hk, v.x, acc[r].x);
            acc[r].y = fmaf(hk, v.y, acc[r].y);
        }
    }
}

// Four samples j .. j + 3 (j a multiple of 4: no pad between them) that EVERY output takes, and their kDdcR x 4 taps
struct DdcChunk {
    float2 v[4];
    float h[kDdcR][4];
};
__device__ __forceinline__ void ddc_load4(DdcChunk &c, const float2 *at, const __attribute__((address_space(4))) float *h, int j, int D) {
#pragma unroll
    for (int u = 0; u < 4; ++u) c.v[u] = at[u];
#pragma unroll
    for (int r = 0; r < kDdcR; ++r)
#pragma unroll
        for (int u = 0; u < 4; ++u) c.h[r][u] = h[j - r * D + u];
}
__device__ __forceinline__ void ddc_feed4(float2 (&acc)[kDdcR], const DdcChunk &c) {
#pragma unroll
    for (int u = 0; u < 4; ++u) // ascending j is ascending k for every output
#pragma unroll
        for (int r = 0; r < kDdcR; ++r) {
            acc[r].x = fmaf(c.h[r][u], c.v[u].x, acc[r].x);
            acc[r].y = fmaf(c.h[r][u], c.v[u].y, acc[r].y);
        }
}

template <bool SC16> __global__ __launch_bounds__(256) void k_ddc(DdcLaunch a) {
    __shared__ float2 s_v[kDdcLds];
    const DdcParams &p = a.p;
    const int D = p.decim, T = p.n_taps, RD = kDdcR * D;
    constexpr int W = SC16 ? 4 : 2; // samples in 16 bytes
    const auto *h = (const __attribute__((address_space(4))) float *)p.taps;
    for (long long u = blockIdx.x; u < a.units; u += gridDim.x) {
        if (u >= a.tiles) { // the carry behind the piece
            const long long i = a.c1 + (u - a.tiles) * 256 + threadIdx.x;
            if (i < p.t0 + p.n) p.carry_new[i - a.c1] = ddc_raw<SC16>(a, i);
            continue;
        }
        const long long m_lo = a.m0 + u * a.tile;
        const int n_out = (int)(m_lo + a.tile < a.m1 ? a.tile : a.m1 - m_lo);
        const long long i_lo = m_lo * D;
        const int span = n_out * D + T - D; // the samples under the tile: i_lo .. i_lo + span - 1, all of them in front of t0 + n
        // the part in front of the piece
        const int n_carry = (int)(p.t0 > i_lo ? (p.t0 - i_lo < span ? p.t0 - i_lo : span) : 0);
        for (int s = threadIdx.x; s < n_carry; s += 256) s_v[ddc_pos(a, s)] = ddc_mix(p, p.carry_old[i_lo + s - a.c0], i_lo + s);
        // the part inside it: piece elements e_lo .. e_hi - 1, in groups of 16 bytes on `in`'s own grid
        const long long e_lo = i_lo + n_carry - p.t0, e_hi = i_lo + span - p.t0;
        for (long long g = (e_lo + a.mis) / W + threadIdx.x; g * W - a.mis < e_hi; g += 256) {
            const long long e0 = g * W - a.mis;
            const int s0 = (int)(e0 + p.t0 - i_lo);
            if (e0 >= e_lo && e0 + W <= e_hi) {
                float2 x[W];
                if constexpr (SC16) {
                    const uint4 d = *reinterpret_cast<const uint4 *>(static_cast<const uint32_t *>(p.in) + e0);
                    x[0] = sc16_widen1(d.x, p.scale); x[1] = sc16_widen1(d.y, p.scale);
                    x[2] = sc16_widen1(d.z, p.scale); x[3] = sc16_widen1(d.w, p.scale);
                } else {
                    const float4 d = *reinterpret_cast<const float4 *>(static_cast<const float2 *>(p.in) + e0);
                    x[0] = make_float2(d.x, d.y); x[1] = make_float2(d.z, d.w);
                }
#pragma unroll
                for (int q = 0; q < W; ++q) s_v[ddc_pos(a, s0 + q)] = ddc_mix(p, x[q], p.t0 + e0 + q);
            } else {
                for (long long e = e0 > e_lo ? e0 : e_lo; e < e0 + W && e < e_hi; ++e)
                    s_v[ddc_pos(a, (int)(e + p.t0 - i_lo))] = ddc_mix(p, ddc_raw<SC16>(a, p.t0 + e), p.t0 + e);
            }
        }
        __syncthreads();
        const int t = threadIdx.x;
        if (t * kDdcR < n_out) {
            // sample j under this thread's outputs lies at base[j + j / RD]; outputs behind n_out read slots of the image that
            // nothing staged and are not stored
            const float2 *base = s_v + t * (RD + 1);
            float2 acc[kDdcR];
#pragma unroll
            for (int r = 0; r < kDdcR; ++r) acc[r] = make_float2(0.f, 0.f);
            const int j_end = (kDdcR - 1) * D + T;
            const int full_lo = (kDdcR - 1) * D < T ? (kDdcR - 1) * D : T, full_hi = T; // every output takes sample j for full_lo <= j < full_hi
            int j = 0, off = 0, q = 0; // off = j + j / RD, q = j % RD
            for (; j < full_lo || ((j & 3) && j < j_end); ++j) { // up to the first multiple of 4 from which every output takes every sample
                ddc_feed<true>(acc, base[off], h, j, D, T);
                ++off;
                if (++q == RD) { q = 0; ++off; }
            }
            if (j + 4 <= full_hi) { // four samples a step, the next step's samples and taps in flight while this step's are used
                DdcChunk cur;
                ddc_load4(cur, base + off, h, j, D);
                for (;;) {
                    j += 4; off += 4; q += 4;
                    if (q == RD) { q = 0; ++off; } // RD is a multiple of 4
                    if (j + 4 > full_hi) break;
                    DdcChunk nxt;
                    ddc_load4(nxt, base + off, h, j, D);
                    ddc_feed4(acc, cur);
                    cur = nxt;
                }
                ddc_feed4(acc, cur);
            }
            for (; j < j_end; ++j) {
                ddc_feed<true>(acc, base[off], h, j, D, T);
                ++off;
                if (++q == RD) { q = 0; ++off; }
            }
            float2 *o = p.out + (m_lo - a.m0) + t * kDdcR;
#pragma unroll
            for (int r = 0; r < kDdcR; ++r)
                if (t * kDdcR + r < n_out) o[r] = acc[r];
        }
        __syncthreads(); // the next tile of this workgroup overwrites the image
    }
}

hipError_t run_ddc(const DdcParams &p, bool sc16, int num_cu, hipStream_t st) {
    if (p.n < 0 || p.t0 < 0 || p.decim < 1 || p.decim > kDdcMaxDecim || p.n_taps < p.decim || p.n_taps > kDdcMaxTaps) return hipErrorInvalidValue;
    if (p.n == 0) return hipSuccess;
    if (!p.in || !p.taps || !p.coarse || !p.fine || !p.carry_old || !p.carry_new) return hipErrorInvalidValue;
    const uintptr_t in = reinterpret_cast<uintptr_t>(p.in), ss = sc16 ? 4 : 8;
    // the 16-byte groups rest on this: refuse a caller that broke it rather than fault
    if ((in & (ss - 1)) || (reinterpret_cast<uintptr_t>(p.out) & 7)) return hipErrorInvalidValue;
    DdcLaunch a;
    a.p = p;
    a.m0 = ddc_out_len(p.t0, p.decim, p.n_taps);
    a.m1 = ddc_out_len(p.t0 + p.n, p.decim, p.n_taps);
    if (a.m1 > a.m0 && !p.out) return hipErrorInvalidValue;
    a.c0 = a.m0 * p.decim;
    a.c1 = a.m1 * p.decim;
    const int RD = kDdcR * p.decim;
    a.rd_magic = (unsigned)(((1ull << 32) + RD - 1) / RD);
    a.mis = (int)((in & 15) / ss);
    // the largest tile whose image fits: span + span / RD <= kDdcLds with span = tile D + T - D, i.e. span <= kDdcLds RD / (RD + 1)
    const long long span_max = (long long)kDdcLds * RD / (RD + 1);
    long long tile = (span_max - (p.n_taps - p.decim)) / p.decim / kDdcR * kDdcR;
    if (tile > 256 * kDdcR) tile = 256 * kDdcR;
    if (tile < kDdcR) return hipErrorInvalidValue; // never: kDdcLds holds one thread's outputs at D = 64, T = 4096
    a.tile = (int)tile;
    a.tiles = (a.m1 - a.m0 + tile - 1) / tile;
    a.units = a.tiles + (p.t0 + p.n - a.c1 + 255) / 256;
    // three workgroups are resident on a CU (the 48 KiB image); the grid is what is resident, the loop strides over the rest
    const dim3 grid((unsigned)persistent_grid(a.units, (long long)num_cu * 3, tuning_or_default(p.tune)));
    trace_add(p.trace, sc16 ? "k_ddc<sc16>" : "k_ddc<fc32>");
    if (sc16) hipLaunchKernelGGL(k_ddc<true>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_ddc<false>, grid, dim3(256), 0, st, a);
    return hipGetLastError();
}

} // namespace ofdm
