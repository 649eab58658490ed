// kernels_quality.hip -- EXT-6 link quality (ofdm_rx_quality_batch; definition: tests/quality_ref.py, include/ofdm_hip.h).
//
// One symbol slot (T = N/8 threads, 8 points per thread, as in kernels_sym.hip) OWNS a frame and walks it: the five training blocks
// (read once, the next block's loads in flight; the noise sum forms on the way from deviations against the running mean), one FFT of
// their sum, then the frame's counted data symbols one after another, the next
// symbol's loads in flight while this one runs its passes.  The frame's six sums stay in the slot's registers -- per thread serially
// over blocks / symbols, then one symbol_sum tree each -- and leave once, as one row written by one thread: no atomics, no zeroed
// counters, no second launch, and the row's bits depend neither on the grid nor on the frames that share the wavefront.
//
// For N <= 512 several frames share a wavefront: the symbol loop runs to the MAXIMUM of the wavefront's slots (for T > 64 of the
// workgroup's: the passes and sums there go through barriers), and a slot whose frame is finished, dead or cut contributes nothing
// (the dead-symbol rule).
#include "../../include/ofdm_hip.h" // the row's field indices OFDM_Q_*
#include "device_common.hpp"
#include "kernels.hpp"

namespace ofdm {

static_assert(kQualityFields == OFDM_QUALITY_FIELDS, "the row of include/ofdm_hip.h");

template <int N>
__global__ __launch_bounds__(Plan<N>::WG) void k_linkq(LinkqParams p) {
    typedef Plan<N> P;
    constexpr int T = P::T, G = P::G;
    constexpr int K = N / 64; // carrier-map tiling factor (EXT-4)

    __shared__ cf lds[G * P::LDS_SYM];
    __shared__ float red[(T > 64) ? G * (T / 64) : 1];
    __shared__ int trips[(T > 64) ? G : 1];

    const int tid = threadIdx.x;
    const int t = tid % T, slot = tid / T;
    cf *buf = lds + slot * P::LDS_SYM;

    cf w[P::NTW > 0 ? P::NTW : 1];
    load_twiddles<N>(p.tw, t, w);

    const int S = p.sym_len;     // N + CP
    const int cp = S - N;
    const int c0 = t / K;        // reference carrier class of bin t + m*T is c0 + 8m
    const int nd = p.guard ? 48 * K : N;
    const long long pts_max = (long long)p.syms_per_frame * nd;

    // the eight samples x[t + m*T] of an N-point window that starts at `at` - t.  A window is only ever wanted when it lies wholly inside
    // the capture (a counted training part, a counted data symbol), so one verdict serves its eight loads and they share one address.
    auto fetch = [&](const cf *at, bool want, cf *dst) {
        if (want) {
#pragma unroll
            for (int m = 0; m < 8; ++m) dst[m] = at[m * T];
        } else {
#pragma unroll
            for (int m = 0; m < 8; ++m) dst[m] = make_float2(0.f, 0.f);
        }
    };

    for (long long base = (long long)blockIdx.x * G; base < p.n_frames; base += (long long)gridDim.x * G) {
        const long long f = base + slot;
        const bool alive = f < p.n_frames && !(p.status && p.status[f] != 0);
        const long long off = (alive && p.offset) ? p.offset[f] : 0;
        const double turns = (alive && p.f_delta) ? p.f_delta[f] * 0.15915494309189533577 : 0.0; // 1/(2 pi)
        const cf *src = p.in + (alive ? f : 0) * p.frame_stride + (alive ? off : 0) + cp + t; // sample n = t of symbol 0's FFT window
        // the training part counts only with all five blocks inside the capture; without it the whole row is 0
        const bool trained = alive && off >= 0 && off + 10LL * S <= p.frame_len;
        // counted data symbols: those that hold one of the frame's n_points points and lie wholly inside the capture
        long long npts = (trained && p.n_points) ? p.n_points[f] : 0;
        npts = npts < 0 ? 0 : (npts > pts_max ? pts_max : npts);
        int mine = 0;
        if (npts > 0) {
            const long long whole = (p.frame_len - off) / S - p.first_symbol; // symbols k with off + (first_symbol + k + 1) S <= frame_len
            const long long need = (npts + nd - 1) / nd;
            mine = (int)(whole < need ? (whole < 0 ? 0 : whole) : need);
        }

        // ------------------------------------------------------------------ training blocks 5 .. 9
        // One pass (Welford): with A_b the sum of blocks 0 .. b, sum_b |y_b - ybar|^2 = sum_{b >= 1} Re (y_b - A_{b-1} / b) conj(y_b - A_b / (b + 1)),
        // every term a product of two deviations from a running mean -- as well conditioned as the two-pass form, which would hold all 40
        // samples of a thread (80 VGPRs) or read and derotate them twice.  acc is summed in k_sym<chest>'s order: FFT(acc) is the
        // quantity it divides by the training table.
        // The loop stays rolled, the next block's loads in flight while this one is derotated and added: unrolled, the compiler issues all
        // 40 loads of a thread first and the kernel spills.  Block 0 goes through the same lines with A_{-1} = 0 and adds 0.
        cf acc[8], nxt[8];
        float s_noise = 0.f;
        const cf st = cfo_phasor(turns, T);
#pragma unroll
        for (int m = 0; m < 8; ++m) acc[m] = make_float2(0.f, 0.f);
        fetch(src + 5LL * S, trained, nxt);
#pragma unroll 1
        for (int b = 0; b < 5; ++b) {
            cf y[8];
#pragma unroll
            for (int m = 0; m < 8; ++m) y[m] = nxt[m];
            fetch(src + (long long)(6 + b) * S, trained && b < 4, nxt);
            if (p.f_delta) { // derotation as in k_sym<chest>: the sample id counts from the frame's offset
                cf ph = cfo_phasor(turns, (long long)(5 + b) * S + cp + t);
#pragma unroll
                for (int m = 0; m < 8; ++m) { y[m] = cmul(y[m], ph); ph = cmul(ph, st); }
            }
            const float ro = b == 0 ? 0.f : b == 1 ? 1.f : b == 2 ? 0.5f : b == 3 ? (1.0f / 3.0f) : 0.25f;         // 1 / b
            const float rn = b == 0 ? 1.f : b == 1 ? 0.5f : b == 2 ? (1.0f / 3.0f) : b == 3 ? 0.25f : 0.2f;        // 1 / (b + 1)
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                const float ox = fmaf(-ro, acc[m].x, y[m].x), oy = fmaf(-ro, acc[m].y, y[m].y);
                acc[m] = cadd(acc[m], y[m]);
                const float nx = fmaf(-rn, acc[m].x, y[m].x), ny = fmaf(-rn, acc[m].y, y[m].y);
                s_noise = fmaf(ox, nx, fmaf(oy, ny, s_noise));
            }
        }
        cf pre[8]; // the first data symbol's loads go out before the training blocks' FFT
        fetch(src + (long long)p.first_symbol * S, mine > 0, pre);
        fft_symbol<N, false>(acc, buf, t, w);
        float s_sig = 0.f; // sum over the data carriers of |FFT(sum of the blocks)|^2 = 25 |Ybar|^2
#pragma unroll
        for (int m = 0; m < 8; ++m)
            if (carrier_class64(c0 + 8 * m, p.guard) == 0) s_sig = fmaf(acc[m].x, acc[m].x, fmaf(acc[m].y, acc[m].y, s_sig));

        // ------------------------------------------------------------------ the caller's channel estimate
        cf hh[8];
        float rn[8], s_h2 = 0.f;
        if (p.hk) {
            const cf *h = p.hk + (trained ? f : 0) * p.hk_stride;
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                hh[m] = trained ? h[t + m * T] : make_float2(1.f, 0.f);
                const float n2 = hh[m].x * hh[m].x + hh[m].y * hh[m].y;
                rn[m] = __builtin_amdgcn_rcpf(n2); // as k_sym<demod>
                if (carrier_class64(c0 + 8 * m, p.guard) == 0) s_h2 += n2;
            }
        }

        // ------------------------------------------------------------------ data symbols: decision-directed EVM
        int trip = mine;
        if (T > 64) {
            __syncthreads();
            if (t == 0) trips[slot] = mine;
            __syncthreads();
#pragma unroll
            for (int g = 0; g < G; ++g) trip = max(trip, trips[g]);
        } else {
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) trip = max(trip, __shfl_xor(trip, s, 64));
        }
        float s_err = 0.f, s_ref = 0.f, s_cnt = 0.f;
        for (int k = 0; k < trip; ++k) {
            const bool live = k < mine;
            cf v[8];
#pragma unroll
            for (int m = 0; m < 8; ++m) v[m] = pre[m];
            fetch(src + (long long)(p.first_symbol + k + 1) * S, k + 1 < mine, pre); // the next symbol's loads, issued now
            if (p.f_delta && live) {
                cf ph = cfo_phasor(turns, (long long)(p.first_symbol + k) * S + cp + t);
#pragma unroll
                for (int m = 0; m < 8; ++m) { v[m] = cmul(v[m], ph); ph = cmul(ph, st); }
            }
            fft_symbol<N, false>(v, buf, t, w);
            // equalise and rotate by the mean pilot angle exactly as k_sym<demod> does for soft_dev
            if (p.hk && live) {
#pragma unroll
                for (int m = 0; m < 8; ++m) {
                    const cf q = cmulc(v[m], hh[m]);
                    v[m] = make_float2(q.x * rn[m], q.y * rn[m]);
                }
            }
            if (p.guard) {
                float ang = 0.f; // in units of pi
#pragma unroll
                for (int m = 0; m < 8; ++m)
                    if (carrier_class64(c0 + 8 * m, 1) == 2) ang += __ocml_atan2pi_f32(v[m].y, v[m].x);
                ang = symbol_sum<T>(ang, red, slot, t) / (4.0f * K);
                float s, c;
                sincospif(ang, &s, &c);
                const cf rot = make_float2(c, -s);
#pragma unroll
                for (int m = 0; m < 8; ++m) v[m] = cmul(v[m], rot);
            }
            if (live) {
#pragma unroll
                for (int m = 0; m < 8; ++m) {
                    const int c = c0 + 8 * m;
                    if (carrier_class64(c, p.guard) == 0) {
                        const int q = p.guard ? data_classes_below64(c) * K + (t % K) : (t + m * T);
                        if ((long long)k * nd + q < npts) { // padding points behind the frame's last one are not counted
                            const cf xh = map_point(demap_point(v[m], p.bps), p.bps);
                            const float dx = v[m].x - xh.x, dy = v[m].y - xh.y;
                            s_err = fmaf(dx, dx, fmaf(dy, dy, s_err));
                            s_ref = fmaf(xh.x, xh.x, fmaf(xh.y, xh.y, s_ref));
                            s_cnt += 1.0f;
                        }
                    }
                }
            }
        }

        // ------------------------------------------------------------------ the row
        const float noise = symbol_sum<T>(s_noise, red, slot, t) * 0.25f;
        const float sig = symbol_sum<T>(s_sig, red, slot, t);
        const float h2 = p.hk ? symbol_sum<T>(s_h2, red, slot, t) / (float)nd : 1.0f;
        const float err = symbol_sum<T>(s_err, red, slot, t);
        const float ref = symbol_sum<T>(s_ref, red, slot, t);
        const float cnt = symbol_sum<T>(s_cnt, red, slot, t);
        if (t == 0 && f < p.n_frames) {
            float row[kQualityFields] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (trained) {
                const int M = p.bps <= 2 ? 2 : 1 << (p.bps >> 1);
                const float gain = (sig * 0.04f - (float)nd * (noise * 0.2f)) * p.inv_t2;
                row[OFDM_Q_VALID] = 1.f;
                row[OFDM_Q_NOISE_VAR] = noise;
                row[OFDM_Q_GAIN] = gain;
                row[OFDM_Q_SNR] = noise == 0.f ? __builtin_inff() : fmaxf(gain, 0.f) * p.es / noise;
                row[OFDM_Q_LLR_UNIT] = 4.0f * h2 / ((float)((M - 1) * (M - 1)) * noise);
                row[OFDM_Q_EVM2] = cnt > 0.f ? err / ref : 0.f;
                row[OFDM_Q_POINTS] = cnt;
            }
            float *dst = p.quality + f * kQualityFields; // (the caller's rows need no alignment)
#pragma unroll
            for (int i = 0; i < kQualityFields; ++i) dst[i] = row[i];
        }
    }
}

template <int N> static hipError_t launch_linkq(const LinkqParams &p, hipStream_t st, int num_cu) {
    typedef Plan<N> P;
    if (p.n_frames <= 0) return hipSuccess;
    // persistent: ~8 workgroups per CU, grid-stride over groups of G frames
    const int grid = (int)persistent_grid((p.n_frames + P::G - 1) / P::G, (long long)num_cu * 8, tuning_or_default(p.tune));
    trace_add(p.trace, "k_linkq");
    hipLaunchKernelGGL((k_linkq<N>), dim3(grid), dim3(P::WG), 0, st, p);
    return hipGetLastError();
}

float linkq_inv_t2(const double *training, int n, int guard) {
    double t2 = 0.0; // summed in f64 on the host, once per call
    for (int k = 0; k < n; k++)
        if (carrier_class64(k / (n / 64), guard) == 0) t2 += training[2 * k] * training[2 * k] + training[2 * k + 1] * training[2 * k + 1];
    return (float)(1.0 / t2);
}
float linkq_es(int bps) {
    if (bps <= 2) return (float)bps; // BPSK: 1, QPSK: 2 (points +-1 +-j)
    const double M = (double)(1 << (bps >> 1));
    return (float)(2.0 * (M + 1.0) / (3.0 * (M - 1.0)));
}

hipError_t run_linkq(int n, const LinkqParams &p, hipStream_t st, int num_cu) {
    const hipError_t e = with_int<64, 128, 256, 512, 1024, 2048, 4096>(n, [&](auto N) { return launch_linkq<decltype(N)::value>(p, st, num_cu); });
    return e == hipErrorNotSupported ? hipErrorInvalidValue : e;
}

} // namespace ofdm
