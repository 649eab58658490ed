// kernels_noise.hip -- EXT-11 noise-aware LLR weights, the per-carrier noise estimate (ofdm_rx_noise_bins_batch and the
// OFDM_LLRW_NOISE receive mode; definition: tests/noise_weight_ref.py, include/ofdm_hip.h).
//
// The five training blocks are identical, so their scatter is the noise; k_linkq sums it over all bins into one noise_var, here it is
// kept per bin: s_k = (1/4) sum_b |FFT(y_b - ybar)[k]|^2, and the weight q_k = min(1, mean(s) / s_k) that k_sym<llrw> multiplies into
// the LLR scale of bin k.
//
// The mapping is k_linkq's and k_cfo_wide's: one symbol slot (T = N/8 threads, 8 points per thread) OWNS a frame.  It reads the five
// blocks once and keeps all 40 derotated samples of a thread in registers (this kernel needs every block again after their mean is
// known, and a second read would derotate twice); the deviations from the mean are formed in the time domain, before any transform, so
// the rounding error of s_k is relative to s_k and not to the signal's |Y_k|^2.  Five FFTs, the powers summed per bin in registers, one
// symbol_sum tree for the mean, and every thread writes its eight bins of the row: no atomics, no zeroed counters, no second launch, no
// workspace, and a frame's bits depend neither on the grid nor on the frames that share its wavefront or workgroup.
//
// Slots that share a wavefront (N <= 512) or a workgroup (N >= 1024) walk the same five transforms, so every barrier and shuffle is
// uniform; a frame that is not tested loads nothing and carries zeros through them (the dead-symbol rule), which
// gives s = 0 and q = 1 by the same lines that serve a tested frame.
#include "device_common.hpp"
#include "kernels.hpp"

namespace ofdm {

template <int N>
__global__ __launch_bounds__(Plan<N>::WG) void k_noise_bins(NoiseBinsParams p) {
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

    for (long long base = (long long)blockIdx.x * G; base < p.n_frames; base += (long long)gridDim.x * G) {
        const long long f = base + slot;
        const bool alive = f < p.n_frames && !(p.status && p.status[f] != 0);
        const long long off = alive ? p.offset[f] : 0;
        // tested only with all five training blocks inside the capture
        const bool tested = alive && off >= 0 && off + 10LL * S <= p.frame_len;
        const double turns = (tested && p.f_delta) ? p.f_delta[f] * 0.15915494309189533577 : 0.0; // 1/(2 pi)
        const cf *src = p.in + (tested ? f * p.frame_stride + off : 0) + cp + t; // sample n = t of symbol 0's FFT window

        // ------------------------------------------------------------------ training blocks 5 .. 9, derotated as in k_sym<chest>
        cf y[5][8];
#pragma unroll
        for (int b = 0; b < 5; ++b) {
            if (tested) {
                const cf *at = src + (long long)(5 + b) * S;
#pragma unroll
                for (int m = 0; m < 8; ++m) y[b][m] = at[m * T];
            } else {
#pragma unroll
                for (int m = 0; m < 8; ++m) y[b][m] = make_float2(0.f, 0.f);
            }
        }
        if (p.f_delta) {
            const cf st = cfo_phasor(turns, T);
#pragma unroll
            for (int b = 0; b < 5; ++b) {
                cf ph = cfo_phasor(turns, (long long)(5 + b) * S + cp + t); // the sample id counts from the frame's offset
#pragma unroll
                for (int m = 0; m < 8; ++m) { y[b][m] = cmul(y[b][m], ph); ph = cmul(ph, st); }
            }
        }

        // ------------------------------------------------------------------ deviations from the mean, in the time domain
        // d_b = y_b - ybar as the mean of the differences y_b - y_c: every term is a deviation, and five identical blocks (a noiseless
        // frame) give exactly 0, which a rounded mean would not
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            cf d[5];
#pragma unroll
            for (int b = 0; b < 5; ++b) {
                cf a = make_float2(0.f, 0.f);
#pragma unroll
                for (int c = 0; c < 5; ++c)
                    if (c != b) a = cadd(a, csub(y[b][m], y[c][m]));
                d[b] = make_float2(a.x * 0.2f, a.y * 0.2f);
            }
#pragma unroll
            for (int b = 0; b < 5; ++b) y[b][m] = d[b];
        }

        // ------------------------------------------------------------------ s_k = (1/4) sum_b |FFT(d_b)[k]|^2 at the bins k = t + m T
        float s[8];
#pragma unroll
        for (int m = 0; m < 8; ++m) s[m] = 0.f;
#pragma unroll
        for (int b = 0; b < 5; ++b) {
            fft_symbol<N, false>(y[b], buf, t, w);
#pragma unroll
            for (int m = 0; m < 8; ++m) s[m] = fmaf(y[b][m].x, y[b][m].x, fmaf(y[b][m].y, y[b][m].y, s[m]));
        }
        float part = 0.f;
#pragma unroll
        for (int m = 0; m < 8; ++m) { s[m] *= 0.25f; part += s[m]; }
        const float sbar = symbol_sum<T>(part, red, slot, t) * (1.0f / (float)N); // (a power of two: exact)

        // ------------------------------------------------------------------ the rows: q_k = sbar / s_k where s_k > sbar (false for NaN), else 1
        if (f < p.n_frames) {
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                if (p.nvar) p.nvar[f * N + t + m * T] = s[m];
                if (p.weight) p.weight[f * N + t + m * T] = s[m] > sbar ? sbar / s[m] : 1.0f;
            }
        }
    }
}

template <int N> static hipError_t launch_noise_bins(const NoiseBinsParams &p, hipStream_t st, int num_cu) {
    typedef Plan<N> P;
    if (p.n_frames <= 0) return hipSuccess;
    // persistent: ~8 workgroups per CU, grid-stride over groups of G frames
    const int grid = (int)persistent_grid((p.n_frames + P::G - 1) / P::G, (long long)num_cu * 8, tuning_or_default(p.tune));
    trace_add(p.trace, "k_noise_bins");
    hipLaunchKernelGGL((k_noise_bins<N>), dim3(grid), dim3(P::WG), 0, st, p);
    return hipGetLastError();
}

hipError_t run_noise_bins(int n, const NoiseBinsParams &p, hipStream_t st, int num_cu) {
    const hipError_t e = with_int<64, 128, 256, 512, 1024, 2048, 4096>(n, [&](auto N) { return launch_noise_bins<decltype(N)::value>(p, st, num_cu); });
    return e == hipErrorNotSupported ? hipErrorInvalidValue : e;
}

} // namespace ofdm
