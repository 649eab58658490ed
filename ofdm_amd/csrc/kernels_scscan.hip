// kernels_scscan.hip -- EXT-12: every Schmidl-Cox detection of one long capture in one pass (ofdm_sc_scan_long).  Definition:
// include/ofdm_hip.h ("every packet of one long capture"); numpy restatement: tests/scan_ref.py.
//   k_sc_mark    one bit per lag of [lag_lo, lag_hi): den > 0 && num >= thr den.  Bit d - lag_lo lives in word (d - lag_lo) >> 6.
//   k_sc_walk    one wavefront walks the bitmap: d1_0 = the first set bit, d1_{k+1} = the first set bit at or after d1_k + holdoff.
//   k_sc_peaks   one workgroup per detection: the first maximum of M over [d1_k, min(d1_k + W, valid - 1)], its CFO and metric.
// Every lag's P, E, R are the oracle's own (sc_at): one thread adds the window's W product pairs in order (acc, sc_common.hpp), from
// that window's samples alone.  So a decision depends on the lag and the capture only -- not on the grid, the tiling, lag_lo or on
// anything that slid through earlier samples -- and it is the f64 CPU oracle's at any margin and any dynamic range
// (tests/sc_margin_cases.py) without a second look.  The price is W pairs per lag instead of one: 12 f64-rate VALU operations per pair,
// which is what bounds k_sc_mark (the window's samples come from L1 / L2: a wavefront's 64 lags read 64 consecutive samples per step).
// No LDS staging, no atomics, no workspace but the bitmap; every store is a vector store.
#include "sc_common.hpp"
#include "kernels.hpp"

namespace ofdm {

constexpr int kScanWg = 256; // k_sc_mark / k_sc_peaks: four wavefronts; a wavefront of k_sc_mark owns one bitmap word

// The oracle's sums at one lag: a = the window's first sample (sc_direct of kernels_sync.hip on global memory).  Reads a[0 .. W + L).
__device__ __forceinline__ ScSums scan_sums(const cf *__restrict__ a, int L, int W) {
    ScSums y = ScSums{0, 0, 0, 0};
#pragma unroll 4
    for (int m = 0; m < W; ++m) y = acc(y, a[m], a[m + L]);
    return y;
}

// Reads in[lag_lo .. lag_lo + n_lags - 1 + W + L): the caller guarantees lag_lo + n_lags <= valid = n_samples - W - L + 1.  Writes
// bits[0 .. ceil(n_lags / 64)): every word whole, the bits of lags at or beyond n_lags zero.
__global__ __launch_bounds__(kScanWg) void k_sc_mark(ScScanParams p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long n_words = (p.n_lags + 63) >> 6;
    for (long long w = (long long)blockIdx.x * (kScanWg / 64) + wave; w < n_words; w += (long long)gridDim.x * (kScanWg / 64)) {
        const long long j = (w << 6) + lane; // lag - lag_lo
        bool hit = false;
        if (j < p.n_lags) {
            const ScSums y = scan_sums(p.in + p.lag_lo + j, p.L, p.W);
            const double den = __dmul_rn(y.e, y.r);
            hit = den > 0.0 && sc_num(y) >= __dmul_rn(p.threshold, den);
        }
        const unsigned long long word = __ballot(hit);
        if (lane == 0) p.bits[w] = word;
    }
}

// One wavefront.  64 words per step: lane i holds word base + i, a ballot finds the first word with a set bit at or after `pos`,
// count-trailing-zeros the bit; the words stay in registers while the next search start lies inside them.  Writes d1[0 .. n_det) and
// head = {n_det, more}; n_det <= det_cap.
__global__ __launch_bounds__(64) void k_sc_walk(ScScanParams p) {
    const int lane = threadIdx.x;
    const long long n_bits = p.n_lags, n_words = (n_bits + 63) >> 6;
    long long pos = 0, n_det = 0, more = 0;
    bool open = true;
    while (open && pos < n_bits) {
        const long long base = pos >> 6, wi = base + lane;
        const unsigned long long word = wi < n_words ? p.bits[wi] : 0ull;
        const long long end = (base + 64) << 6;
        while (pos < end && pos < n_bits) {
            const long long pw = pos >> 6;
            const unsigned long long v = wi < pw ? 0ull : (wi == pw ? word & (~0ull << (pos & 63)) : word);
            const unsigned long long any = __ballot(v != 0ull);
            if (!any) { pos = end; break; }
            const int first = __builtin_ctzll(any);
            const long long d = ((base + first) << 6) + __builtin_ctzll(__shfl(v, first, 64));
            if (n_det == p.det_cap) { more = 1; open = false; break; }
            if (lane == 0) p.d1[n_det] = p.lag_lo + d;
            ++n_det;
            pos = d + p.holdoff;
        }
    }
    if (lane == 0) { p.head[0] = n_det; p.head[1] = more; }
}

// One workgroup per detection (persistent over head[0] detections).  Reads in[d1 .. last + W + L), last = min(d1 + W, valid - 1), so
// nothing at or beyond n_samples; writes row k of d_hat / f_delta / metric.
__global__ __launch_bounds__(kScanWg) void k_sc_peaks(ScScanParams p) {
    __shared__ ScCand wbest[kScanWg / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long n_det = p.head[0];
    for (long long k = blockIdx.x; k < n_det; k += gridDim.x) {
        const long long d1 = p.d1[k];
        const long long last = d1 + p.W < p.valid - 1 ? d1 + p.W : p.valid - 1;
        const int count = (int)(last - d1) + 1;
        ScCand best = ScCand{-1.0, 1.0, 0.0, 0.0, -1};
        for (int j = tid; j < count; j += kScanWg) { // a thread's lags rise: a later one wins only if strictly greater
            const ScSums y = scan_sums(p.in + d1 + j, p.L, p.W);
            const double den = __dmul_rn(y.e, y.r);
            if (den > 0.0) best = cand_pick_ordered(best, ScCand{sc_num(y), den, y.pr, y.pi, j});
        }
        best = cand_wave_best(best);
        __syncthreads(); // the previous detection's wbest has been read
        if (lane == 0) wbest[wave] = best;
        __syncthreads();
        if (tid == 0) {
            ScCand b = wbest[0];
#pragma unroll
            for (int w = 1; w < kScanWg / 64; ++w) b = cand_pick(b, wbest[w]);
            // (d1 itself has den > 0, so there is always a candidate; keep "no detection" rather than a wrong lag otherwise)
            p.d_hat[k] = b.lag < 0 ? -1 : d1 + b.lag;
            p.f_delta[k] = b.lag < 0 ? 0.0 : atan2(b.pi, b.pr) / (double)p.L;
            p.metric[k] = b.lag < 0 ? 0.f : (float)(b.num / b.den);
        }
    }
}

hipError_t run_sc_mark(const ScScanParams &p, int num_cu, hipStream_t st) {
    if (p.n_lags <= 0) return hipSuccess;
    const long long units = (((p.n_lags + 63) >> 6) + kScanWg / 64 - 1) / (kScanWg / 64);
    const dim3 grid((unsigned)persistent_grid(units, (long long)num_cu * resident_blocks(k_sc_mark, kScanWg), tuning_or_default(p.tune)));
    trace_add(p.trace, "k_sc_mark");
    hipLaunchKernelGGL(k_sc_mark, grid, dim3(kScanWg), 0, st, p);
    return hipGetLastError();
}

hipError_t run_sc_scan(const ScScanParams &p, int num_cu, hipStream_t st) {
    if (p.n_lags <= 0) return hipErrorInvalidValue;
    hipError_t e = run_sc_mark(p, num_cu, st);
    if (e != hipSuccess) return e;
    trace_add(p.trace, "k_sc_walk");
    hipLaunchKernelGGL(k_sc_walk, dim3(1), dim3(64), 0, st, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // (launched with no row to write too: it reads head[0] = 0 and leaves)
    const long long rows = p.det_cap > 0 ? p.det_cap : 1;
    const dim3 grid((unsigned)persistent_grid(rows, (long long)num_cu * resident_blocks(k_sc_peaks, kScanWg), tuning_or_default(p.tune)));
    trace_add(p.trace, "k_sc_peaks");
    hipLaunchKernelGGL(k_sc_peaks, grid, dim3(kScanWg), 0, st, p);
    return hipGetLastError();
}

} // namespace ofdm
