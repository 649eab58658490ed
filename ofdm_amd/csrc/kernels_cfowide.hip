// kernels_cfowide.hip -- EXT-8 wide CFO acquisition (ofdm_cfo_wide_batch, OFDM_CFO_WIDE; definition: tests/cfo_wide_ref.py,
// include/ofdm_hip.h).
//
// The Schmidl-Cox phase gives the carrier offset modulo 2 pi / S only.  The five training blocks are one symbol long and identical, so a
// hypothesis m (offset f0 + 2 pi m / S) rotates them all alike, and for the right m their sum, matched against the training table,
// puts its energy into the cp_len delays of the channel window; for a wrong m it spreads over all N.
//
// The mapping is k_linkq's: one symbol slot (T = N/8 threads, 8 points per thread) OWNS a frame.  It reads the five blocks once (the
// next block's loads in flight) and keeps their derotated sum in registers; then, per hypothesis, rotates the sum, transforms it, multiplies
// by conj(t), transforms back and sums |g|^2 over the window with one symbol_sum tree.  The best and the runner-up stay in registers and
// one thread writes the frame's outputs: no atomics, no zeroed counters, no second launch, no workspace, and a frame's bits depend neither
// on the grid nor on the frames that share its wavefront or workgroup.
//
// Slots that share a wavefront (N <= 512) or a workgroup (N >= 1024) walk the same 2 span + 1 hypotheses, so every barrier and
// shuffle is uniform; a dead frame loads nothing and carries zeros through them (the dead-symbol rule).
#include "device_common.hpp"
#include "kernels.hpp"

namespace ofdm {

template <int N>
__global__ __launch_bounds__(Plan<N>::WG) void k_cfo_wide(CfoWideParams p) {
    typedef Plan<N> P;
    constexpr int T = P::T, G = P::G;

    __shared__ cf lds[G * P::LDS_SYM];
    __shared__ float red[(T > 64) ? G * (T / 64) : 1];

    const int tid = threadIdx.x;
    const int t = tid % T, slot = tid / T;
    cf *buf = lds + slot * P::LDS_SYM;

    cf w[P::NTW > 0 ? P::NTW : 1];
    load_twiddles<N>(p.tw, t, w);

    const int S = p.sym_len;     // N + CP
    const int cp = S - N;
    const double inv_s = 1.0 / (double)S;
    constexpr float kScale = (1.0f / (float)N) * (1.0f / (float)N); // g carries the inverse transform's 1 / N (a power of two: exact)

    cf ct[8]; // conj(t) at this thread's bins
#pragma unroll
    for (int k = 0; k < 8; ++k) { const cf v = p.trn[t + k * T]; ct[k] = make_float2(v.x, -v.y); }

    for (long long base = (long long)blockIdx.x * G; base < p.n_frames; base += (long long)gridDim.x * G) {
        const long long f = base + slot;
        const bool alive = f < p.n_frames && !(p.status && p.status[f] != 0);
        const long long off = alive ? p.offset[f] : 0;
        // tested only with all five training blocks inside the capture
        const bool tested = alive && off >= 0 && off + 10LL * S <= p.frame_len;
        const double f0 = tested ? p.f_delta[f] : 0.0;
        const double turns = f0 * 0.15915494309189533577; // 1/(2 pi)
        const cf *src = p.in + (tested ? f * p.frame_stride + off : 0) + cp + t; // sample n = t of symbol 0's FFT window

        // ------------------------------------------------------------------ the sum of training blocks 5 .. 9, in k_sym<chest>'s order
        // The loop stays rolled, the next block's loads in flight while this one is derotated and added (DESIGN.md section 3, EXT-6:
        // unrolled, all 40 loads of a thread are issued first and the kernel spills).
        cf acc[8], nxt[8];
        const cf st = cfo_phasor(turns, T);
#pragma unroll
        for (int k = 0; k < 8; ++k) { acc[k] = make_float2(0.f, 0.f); nxt[k] = make_float2(0.f, 0.f); }
        if (tested) {
#pragma unroll
            for (int k = 0; k < 8; ++k) nxt[k] = src[5LL * S + k * T];
        }
#pragma unroll 1
        for (int b = 0; b < 5; ++b) {
            cf y[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) y[k] = nxt[k];
            if (tested && b < 4) {
                const cf *at = src + (long long)(6 + b) * S;
#pragma unroll
                for (int k = 0; k < 8; ++k) nxt[k] = at[k * T];
            }
            cf ph = cfo_phasor(turns, (long long)(5 + b) * S + cp + t); // the sample id counts from the frame's offset
#pragma unroll
            for (int k = 0; k < 8; ++k) { acc[k] = cadd(acc[k], cmul(y[k], ph)); ph = cmul(ph, st); }
        }

        // ------------------------------------------------------------------ the hypotheses 0, -1, +1, ..., -span, +span
        float best = 0.f, second = -__builtin_inff();
        int m_best = 0;
#pragma unroll 1
        for (int h = 0; h <= 2 * p.span; ++h) {
            const int m = (h & 1) ? -((h + 1) >> 1) : (h >> 1);
            const double mt = (double)m * inv_s; // turns per sample; the phase is reduced in f64 (cfo_phasor)
            cf ph = cfo_phasor(mt, cp + t);
            const cf sm = cfo_phasor(mt, T);
            cf z[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) { z[k] = cmul(acc[k], ph); ph = cmul(ph, sm); }
            fft_symbol<N, false>(z, buf, t, w);
#pragma unroll
            for (int k = 0; k < 8; ++k) z[k] = cmul(z[k], ct[k]);
            fft_symbol<N, true>(z, buf, t, w);
            // the window: delays [-N/16, 3N/16) mod N = points [0, 3T/2) and [N - T/2, N) of z[k] = g[t + k T]
            const cf e1 = t < T / 2 ? z[1] : z[7];
            const float e = fmaf(z[0].x, z[0].x, fmaf(z[0].y, z[0].y, fmaf(e1.x, e1.x, e1.y * e1.y)));
            const float g = symbol_sum<T>(e, red, slot, t) * kScale;
            // kept only if strictly greater; a NaN is never greater and never below the runner-up
            if (h == 0) best = g;
            else if (g > best) { second = best; best = g; m_best = m; }
            else if (!(g <= second)) second = g;
        }

        if (t == 0 && f < p.n_frames) {
            if (p.m) p.m[f] = tested ? m_best : 0;
            if (p.metric) { p.metric[2 * f] = tested ? best : 0.f; p.metric[2 * f + 1] = tested ? second : 0.f; }
            if (tested && m_best != 0) p.f_delta[f] = f0 + (6.283185307179586476925 * (double)m_best) / (double)S; // m = 0: untouched
        }
    }
}

template <int N> static hipError_t launch_cfo_wide(const CfoWideParams &p, hipStream_t st, int num_cu) {
    typedef Plan<N> P;
    if (p.n_frames <= 0) return hipSuccess;
    // persistent: ~8 workgroups per CU, grid-stride over groups of G frames
    const int grid = (int)persistent_grid((p.n_frames + P::G - 1) / P::G, (long long)num_cu * 8, tuning_or_default(p.tune));
    trace_add(p.trace, "k_cfo_wide");
    hipLaunchKernelGGL((k_cfo_wide<N>), dim3(grid), dim3(P::WG), 0, st, p);
    return hipGetLastError();
}

hipError_t run_cfo_wide(int n, const CfoWideParams &p, hipStream_t st, int num_cu) {
    const hipError_t e = with_int<64, 128, 256, 512, 1024, 2048, 4096>(n, [&](auto N) { return launch_cfo_wide<decltype(N)::value>(p, st, num_cu); });
    return e == hipErrorNotSupported ? hipErrorInvalidValue : e;
}

} // namespace ofdm
