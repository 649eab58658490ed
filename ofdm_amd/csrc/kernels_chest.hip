// kernels_chest.hip -- EXT-5 channel-estimate denoising (include/ofdm_hip.h "channel-estimate denoising", DESIGN.md section 3;
// definition: tests/chest_ref.py).  Between the existing k_sym<chest> and the demodulator the estimate of every frame is projected,
// with weights W_k = |t_k|^2, onto channels of L_h = N / 4 taps:
//   k_chest_weight   a_k = W_k H^_k (0 where t_k = 0): the one elementwise pass; it sits in front of the inverse FFT, so it cannot be
//                    folded into the solve kernel's loads
//   k_sym<ifft>      existing generic kernel: g / N in every row's window
//   k_chest_solve    h^ = (N R^-1) (g / N) for a batch: the complex product [n_frames x L_h] . [L_h x L_h], the project's first dense
//                    contraction.  The gather of the window's taps is its load, the scatter into a zeroed row of N taps its store.
//   k_sym<fft>       existing generic kernel: H' = FFT of that row
// k_chest_solve: 256 threads = 16 (taps) x 16 (frames); a workgroup owns a tile of 64 frames x 16 TP output taps, a thread 4 x TP of
// them (frames ty + 16 i, taps tx + 16 j: every LDS read and every store of a quarter wavefront is 16 consecutive float2).  The
// contraction index runs in steps of 16 through LDS: the frames' taps as As[k][frame] (padded row: the transposing store), the matrix
// as Bs[k][tap] from the TRANSPOSED table mt[n][m] = N R^-1[m][n] (coalesced loads, it streams from L2).  The next step's operands
// are fetched into registers while the current one is multiplied.  f32 FMAs in the vector ALU: on gfx950 the f32-input MFMA has the
// same peak, so it would only free issue slots that nothing else here wants.  TP = 4 for L_h >= 64,
// 2 for L_h = 32, 1 for L_h = 16 (N = 64: the whole 16 x 16 matrix is one step).  The sum over n runs in the same order whatever the
// grid: results do not depend on grid_cap.
#include "device_common.hpp"
#include "kernels.hpp"

namespace ofdm {

namespace {
constexpr int kChestKC = 16;     // contraction step
constexpr int kChestTF = 64;     // frames per tile

__global__ __launch_bounds__(256) void k_chest_weight(const float2 *__restrict__ in, const float *__restrict__ w, float2 *out, long long total,
                                                      int mask) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const float wk = w[(int)(i & mask)];
        const float2 h = in[i];
        out[i] = wk == 0.f ? make_float2(0.f, 0.f) : make_float2(wk * h.x, wk * h.y);
    }
}

template <int TP> __global__ __launch_bounds__(256) void k_chest_solve(ChestSolveParams p) {
    constexpr int TM = 16 * TP;
    __shared__ float2 As[kChestKC][kChestTF + 1];
    __shared__ float2 Bs[kChestKC][TM];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int N = p.n_fft, L = p.n_taps, pre = p.pre, nmask = N - 1;
    const int tap_tiles = L / TM;
    const long long frame_tiles = (p.n_frames + kChestTF - 1) / kChestTF, units = frame_tiles * tap_tiles;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const long long ft = u / tap_tiles;
        const int m0 = (int)(u - ft * tap_tiles) * TM;
        const long long f0 = ft * kChestTF;
        float2 acc[4][TP];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < TP; ++j) acc[i][j] = make_float2(0.f, 0.f);
        float2 ra[4], rb[TP];
        auto fetch = [&](int k0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) { // tx = contraction index, ty + 16 i = frame
                const long long f = f0 + ty + 16 * i;
                ra[i] = f < p.n_frames ? p.g[f * N + ((k0 + tx - pre) & nmask)] : make_float2(0.f, 0.f);
            }
#pragma unroll
            for (int j = 0; j < TP; ++j) {
                const int e = t + 256 * j, kk = e / TM, mm = e - kk * TM;
                rb[j] = p.mt[(long long)(k0 + kk) * L + m0 + mm];
            }
        };
        fetch(0);
        for (int k0 = 0; k0 < L; k0 += kChestKC) {
            __syncthreads(); // the previous step's reads are done
#pragma unroll
            for (int i = 0; i < 4; ++i) As[tx][ty + 16 * i] = ra[i];
#pragma unroll
            for (int j = 0; j < TP; ++j) {
                const int e = t + 256 * j, kk = e / TM, mm = e - kk * TM;
                Bs[kk][mm] = rb[j];
            }
            __syncthreads();
            if (k0 + kChestKC < L) fetch(k0 + kChestKC);
#pragma unroll
            for (int k = 0; k < kChestKC; ++k) {
                float2 a[4], b[TP];
#pragma unroll
                for (int i = 0; i < 4; ++i) a[i] = As[k][ty + 16 * i];
#pragma unroll
                for (int j = 0; j < TP; ++j) b[j] = Bs[k][tx + 16 * j];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < TP; ++j) {
                        acc[i][j].x = fmaf(a[i].x, b[j].x, acc[i][j].x);
                        acc[i][j].x = fmaf(-a[i].y, b[j].y, acc[i][j].x);
                        acc[i][j].y = fmaf(a[i].x, b[j].y, acc[i][j].y);
                        acc[i][j].y = fmaf(a[i].y, b[j].x, acc[i][j].y);
                    }
            }
        }
        // tap m goes to index (m - pre) mod N of the row; the 3 L taps outside the window, L - pre + [0, 3 L), are zeroed by the
        // tile that owns m = their position mod L
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long long f = f0 + ty + 16 * i;
            if (f >= p.n_frames) continue;
            float2 *row = p.out + f * N;
#pragma unroll
            for (int j = 0; j < TP; ++j) {
                const int m = m0 + tx + 16 * j;
                row[(m - pre) & nmask] = acc[i][j];
#pragma unroll
                for (int z = 0; z < 3; ++z) row[L - pre + z * L + m] = make_float2(0.f, 0.f);
            }
        }
    }
}
} // namespace

hipError_t run_chest_weight(const float2 *in, const float *w, float2 *out, long long n_frames, int n_fft, int num_cu, const Tuning *tune,
                            hipStream_t st) {
    const long long total = n_frames * n_fft;
    if (total <= 0) return hipSuccess;
    const long long blocks = persistent_grid((total + 255) / 256, 8LL * num_cu, tuning_or_default(tune));
    hipLaunchKernelGGL(k_chest_weight, dim3((unsigned)blocks), dim3(256), 0, st, in, w, out, total, n_fft - 1);
    return hipGetLastError();
}

// Persistent grid of 256 threads, four workgroups per CU: TP = 4 takes 124 VGPRs (four wavefronts per SIMD) and 16.1 KB of LDS
hipError_t run_chest_solve(const ChestSolveParams &p, int num_cu, const Tuning *tune, hipStream_t st) {
    if (p.n_frames <= 0) return hipSuccess;
    const int L = p.n_taps, tp = L >= 64 ? 4 : L / 16;
    if (L < 16 || L % (16 * tp) != 0 || p.n_fft != 4 * L || p.pre < 0 || p.pre > L || p.g == p.out) return hipErrorInvalidValue;
    const long long units = ((p.n_frames + kChestTF - 1) / kChestTF) * (L / (16 * tp));
    const long long blocks = persistent_grid(units, 4LL * num_cu, tuning_or_default(tune));
    return with_int<1, 2, 4>(tp, [&](auto TP) {
        hipLaunchKernelGGL(k_chest_solve<decltype(TP)::value>, dim3((unsigned)blocks), dim3(256), 0, st, p);
        return hipGetLastError();
    });
}

} // namespace ofdm
