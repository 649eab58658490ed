// kernels_stream.hip -- EXT-14: the window of a streaming receiver (ofdm_stream_push; definition: include/ofdm_hip.h, numpy restatement:
// tests/stream_ref.py).
//   k_stream_ingest<fc32>   new[i] = old[drop + i] for i < keep (the carry), new[keep + j] = chunk[j] for j < n
//   k_stream_ingest<sc16>   the same carry, new[keep + j] = (float)chunk[j] * scale per component (sc16_widen1: the product is its own
//                           v_mul_f32, as in k_sc16_widen)
// ONE launch builds the next window: it moves bytes and nothing else, every byte is read once and nothing behind new[keep + n) is written.
// No LDS, no workspace, a persistent grid over tiles of 1024 samples (256 threads x 4 samples), the tiles of the carry in front of
// the tiles of the chunk.  `old + drop` and `new` are 16-byte aligned (the host keeps the window bases on 16 bytes and drop even), so a
// thread of the carry moves its four samples with two 16-byte loads and two 16-byte stores; the chunk side does the same when keep is
// even (then new + keep is on 16 bytes too) and goes sample by sample -- 8-byte stores, 8-byte (fc32) or 4-byte (sc16) loads -- when
// keep is odd.  A tile's ragged tail goes sample by sample on both sides.
#include "device_common.hpp"
#include "kernels.hpp"

namespace ofdm {

constexpr int kIngestTile = 1024; // samples per workgroup step

struct StreamIngestLaunch {
    StreamIngestParams p;
    long long carry_tiles = 0, units = 0;
    int vec = 0; // the chunk side is on 16 bytes (keep is even)
};

template <bool SC16> __global__ __launch_bounds__(256) void k_stream_ingest(StreamIngestLaunch a) {
    const StreamIngestParams &p = a.p;
    for (long long u = blockIdx.x; u < a.units; u += gridDim.x) {
        if (u < a.carry_tiles) {
            const long long i0 = u * kIngestTile + 4 * (long long)threadIdx.x;
            if (i0 + 4 <= p.keep) {
                const float4 x0 = reinterpret_cast<const float4 *>(p.carry + i0)[0], x1 = reinterpret_cast<const float4 *>(p.carry + i0)[1];
                float4 *o = reinterpret_cast<float4 *>(p.win + i0);
                o[0] = x0;
                o[1] = x1;
            } else {
                for (long long i = i0; i < i0 + 4 && i < p.keep; ++i) p.win[i] = p.carry[i];
            }
            continue;
        }
        const long long j0 = (u - a.carry_tiles) * kIngestTile + 4 * (long long)threadIdx.x;
        float2 *dst = p.win + p.keep;
        if constexpr (SC16) {
            const uint32_t *src = static_cast<const uint32_t *>(p.chunk);
            if (a.vec && j0 + 4 <= p.n) {
                const uint4 d = *reinterpret_cast<const uint4 *>(src + j0);
                const float2 s0 = sc16_widen1(d.x, p.scale), s1 = sc16_widen1(d.y, p.scale);
                const float2 s2 = sc16_widen1(d.z, p.scale), s3 = sc16_widen1(d.w, p.scale);
                float4 *o = reinterpret_cast<float4 *>(dst + j0);
                o[0] = make_float4(s0.x, s0.y, s1.x, s1.y);
                o[1] = make_float4(s2.x, s2.y, s3.x, s3.y);
            } else {
                for (long long j = j0; j < j0 + 4 && j < p.n; ++j) dst[j] = sc16_widen1(src[j], p.scale);
            }
        } else {
            const float2 *src = static_cast<const float2 *>(p.chunk);
            if (a.vec && j0 + 4 <= p.n) {
                const float4 x0 = reinterpret_cast<const float4 *>(src + j0)[0], x1 = reinterpret_cast<const float4 *>(src + j0)[1];
                float4 *o = reinterpret_cast<float4 *>(dst + j0);
                o[0] = x0;
                o[1] = x1;
            } else {
                for (long long j = j0; j < j0 + 4 && j < p.n; ++j) dst[j] = src[j];
            }
        }
    }
}

hipError_t run_stream_ingest(const StreamIngestParams &p, bool sc16, int num_cu, hipStream_t st) {
    if (p.keep < 0 || p.n < 0) return hipErrorInvalidValue;
    if (p.keep + p.n == 0) return hipSuccess;
    // the 16-byte paths rest on these: refuse a caller that broke them rather than fault
    if ((reinterpret_cast<uintptr_t>(p.carry) | reinterpret_cast<uintptr_t>(p.win) | reinterpret_cast<uintptr_t>(p.chunk)) & 15) return hipErrorInvalidValue;
    StreamIngestLaunch a;
    a.p = p;
    a.carry_tiles = (p.keep + kIngestTile - 1) / kIngestTile;
    a.units = a.carry_tiles + (p.n + kIngestTile - 1) / kIngestTile;
    a.vec = (p.keep & 1) == 0;
    const dim3 grid((unsigned)persistent_grid(a.units, (long long)num_cu * 8, tuning_or_default(p.tune)));
    trace_add(p.trace, sc16 ? "k_stream_ingest<sc16>" : "k_stream_ingest<fc32>");
    if (sc16) hipLaunchKernelGGL(k_stream_ingest<true>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_stream_ingest<false>, grid, dim3(256), 0, st, a);
    return hipGetLastError();
}

} // namespace ofdm
