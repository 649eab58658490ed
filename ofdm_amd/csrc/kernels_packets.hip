// kernels_packets.hip -- EXT-13: every packet of one long capture through ONE run of the receive chain (ofdm_rx_decode_packets).
// Definition: include/ofdm_hip.h ("every packet of one long capture in one batched decode"); numpy restatement: tests/packets_ref.py.
//   k_pkt_rows         one thread per packet: the row start r_k = max(d_hat_k - L - b, 0) & ~1, the row-relative peak d_hat_k - r_k, the
//                      row's own length min(R, n - r_k), and f_delta_k / M_k where the chain looks for them.
//   k_gather_rows      copies capture[r_k : r_k + R] into row k of the workspace, zeros at and beyond sample n: an ordinary batch of
//                      16-byte aligned rows of R samples (R even), which keeps the rows on the fused frame kernels.
//   k_rx_prepare_rows  rx_prepare_one with the row's own length: a frame cut by the capture's end gets the live symbols of its true
//                      length, and the zeros behind it stand in for pad_chunk -- every later kernel keeps the scalar frame_len = R.
//   k_pkt_finish       row offsets -> int64 offsets into the capture (0 + the row's under OFDM_FRAME_BADTIMING, as ofdm_rx_decode_long).
// No LDS, no atomics; every store is a vector store.  k_gather_rows is bound by bytes: R samples in and out per packet.
#include "device_common.hpp"
#include "kernels.hpp"

namespace ofdm {

constexpr int kPktWg = 256;
constexpr int kGatherPairs = 4;                               // 16-byte pieces (two samples) per thread and step
constexpr int kGatherPiece = kPktWg * kGatherPairs * 2;       // samples per workgroup step: 16 KiB in, 16 KiB out

__global__ __launch_bounds__(kPktWg) void k_pkt_rows(PktParams p) {
    const long long k = (long long)blockIdx.x * kPktWg + threadIdx.x;
    if (k >= p.n_det) return;
    const long long d = p.d_hat[k];
    long long r = d - p.L - p.backoff;
    r = (r < 0 ? 0 : r) & ~1ll;
    const long long left = p.n - r;
    p.row_start[k] = r;
    p.row_dhat[k] = (int32_t)(d - r);                         // <= L + backoff + 1
    p.row_len[k] = (int32_t)(left < p.R ? left : p.R);
    p.f_delta[k] = p.f_delta_in[k];
    if (p.metric) p.metric[k] = p.metric_in[k];
}

// Rows [row0, row0 + n_rows) of the call into rows[0 .. n_rows) (R samples apart).  WIDE: the capture's base is 16-byte aligned, and so
// is every row start (r_k is even): one 16-byte load and store per pair of samples; else 8-byte loads and stores per sample.
// Reads capture[r_k .. min(r_k + R, n)), nothing else; writes rows[row * R .. row * R + R).
template <bool WIDE> __global__ __launch_bounds__(kPktWg) void k_gather_rows(PktParams p) {
    const long long pieces = (p.R + kGatherPiece - 1) / kGatherPiece, units = p.n_rows * pieces;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const long long row = u / pieces, s0 = (u - row * pieces) * kGatherPiece;
        const long long r = p.row_start[p.row0 + row];
        const float2 *src = p.in + r;
        float2 *dst = p.rows + row * p.R;
        const long long live = p.n - r < p.R ? p.n - r : p.R; // samples of the row that the capture holds
#pragma unroll
        for (int i = 0; i < kGatherPairs; ++i) {
            const long long s = s0 + 2 * ((long long)i * kPktWg + threadIdx.x);
            if (s >= p.R) continue;                           // (R is even: a pair is inside the row or outside it)
            if (WIDE) {
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (s + 1 < live) v = *reinterpret_cast<const float4 *>(src + s);
                else if (s < live) { const float2 a = src[s]; v.x = a.x; v.y = a.y; }
                *reinterpret_cast<float4 *>(dst + s) = v;
            } else {
                dst[s] = s < live ? src[s] : make_float2(0.f, 0.f);
                dst[s + 1] = s + 1 < live ? src[s + 1] : make_float2(0.f, 0.f);
            }
        }
    }
}

__global__ __launch_bounds__(kPktWg) void k_rx_prepare_rows(long long n_rows, const int32_t *d_hat, double *f_delta, const int32_t *row_len,
                                                            int L, int backoff, int cfo_mode, int max_symbols, int bytes_per_symbol,
                                                            int32_t *status, int32_t *offset, int32_t *nsym) {
    const long long f = (long long)blockIdx.x * kPktWg + threadIdx.x;
    if (f < n_rows)
        rx_prepare_one(f, d_hat, f_delta, row_len[f], L, backoff, cfo_mode, max_symbols, bytes_per_symbol, status, offset, nsym);
}

__global__ __launch_bounds__(kPktWg) void k_pkt_finish(long long n_det, const long long *row_start, const int32_t *row_offset,
                                                       const int32_t *status, long long *offset) {
    const long long k = (long long)blockIdx.x * kPktWg + threadIdx.x;
    if (k < n_det) offset[k] = (status[k] == -3 ? 0 : row_start[k]) + row_offset[k]; // -3: OFDM_FRAME_BADTIMING
}

hipError_t run_pkt_rows(const PktParams &p, hipStream_t st) {
    if (p.n_det <= 0) return hipSuccess;
    trace_add(p.trace, "k_pkt_rows");
    hipLaunchKernelGGL(k_pkt_rows, dim3((unsigned)((p.n_det + kPktWg - 1) / kPktWg)), dim3(kPktWg), 0, st, p);
    return hipGetLastError();
}

hipError_t run_gather_rows(const PktParams &p, int num_cu, hipStream_t st) {
    if (p.n_rows <= 0 || p.R <= 0) return hipSuccess;
    if ((p.R & 1) || (reinterpret_cast<uintptr_t>(p.rows) & 15) || (reinterpret_cast<uintptr_t>(p.in) & 7)) return hipErrorInvalidValue;
    const bool wide = (reinterpret_cast<uintptr_t>(p.in) & 15) == 0;
    const long long units = p.n_rows * ((p.R + kGatherPiece - 1) / kGatherPiece);
    const Tuning &tu = tuning_or_default(p.tune);
    trace_add(p.trace, "k_gather_rows");
    return with_bool(wide, [&](auto W) {
        constexpr bool kWide = decltype(W)::value;
        const dim3 grid((unsigned)persistent_grid(units, (long long)num_cu * resident_blocks(k_gather_rows<kWide>, kPktWg), tu));
        hipLaunchKernelGGL(k_gather_rows<kWide>, grid, dim3(kPktWg), 0, st, p);
        return hipGetLastError();
    });
}

hipError_t run_rx_prepare_rows(long long n_rows, const int32_t *d_hat, double *f_delta, const int32_t *row_len, int L, int backoff,
                               int cfo_mode, int max_symbols, int bytes_per_symbol, int32_t *status, int32_t *offset, int32_t *nsym,
                               hipStream_t st) {
    if (n_rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_rx_prepare_rows, dim3((unsigned)((n_rows + kPktWg - 1) / kPktWg)), dim3(kPktWg), 0, st, n_rows, d_hat, f_delta,
                       row_len, L, backoff, cfo_mode, max_symbols, bytes_per_symbol, status, offset, nsym);
    return hipGetLastError();
}

hipError_t run_pkt_finish(long long n_det, const long long *row_start, const int32_t *row_offset, const int32_t *status, long long *offset,
                          hipStream_t st) {
    if (n_det <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_pkt_finish, dim3((unsigned)((n_det + kPktWg - 1) / kPktWg)), dim3(kPktWg), 0, st, n_det, row_start, row_offset,
                       status, offset);
    return hipGetLastError();
}

} // namespace ofdm
