// kernels_dcblock.hip -- EXT-15: the DC blocker in front of detection (ofdm_dcblock_push, ofdm_stream_set_dc_block; definition:
// include/ofdm_hip.h "a DC blocker", numpy restatement: tests/dcblock_ref.py).
//   k_dc_block<fc32>   y[i] = x[i] - (float)(mean of the up to M complete 64-sample blocks in front of i's block), block 0 unchanged
//   k_dc_block<sc16>   the same on x = (float)v * scale per component (sc16_widen1: the product is its own v_mul_f32)
// ONE launch per piece of a push filters the piece AND writes the state the next piece reads.  Blocks are aligned at sample 0 of the
// filter's stream, not at the piece: t0 samples lie in front of the piece, the first t0 % 64 of them in the open block the state
// carries as raw samples.  The units of the persistent grid, none of which reads what another writes:
//   tile   tb consecutive blocks (64 for M > 16, else 16).  The sums of the up to M + tb - 1 blocks the tile's means are made of go to LDS,
//          one block a wavefront at a time: a block in front of the piece from the carried ring (slot = block % M), a block inside the
//          piece recomputed from its samples -- lane = sample, f64, the xor-1, 2, 4, 8, 16, 32 butterfly, which is the balanced pairwise
//          tree bit for bit whoever forms it because f64 addition commutes.  Then lane = block: wavefront 0 adds each block's window in
//          ascending order (M sequential f64 additions a lane, M / 64 a sample), divides, rounds once to f32.  Then the tile streams out,
//          four samples a thread, with 16-byte accesses when `in` and `out` are on 16 bytes.
//   ring   (only when the piece completes a block) four ring slots a unit: the sums of the last M blocks into the OTHER copy of the
//          ring, copied or recomputed as above
//   open   the raw samples of the block the piece leaves open, into the OTHER copy of the open block
// The state is double-buffered, so every unit reads the copies the previous launch wrote while this launch writes the others.  No
// atomics; nothing depends on the grid.
#include "device_common.hpp"
#include "kernels.hpp"
#include "wave_ops.hpp"

namespace ofdm {

constexpr int kDcTileMax = 64; // blocks per tile at most: one lane of wavefront 0 per block

struct DcBlockLaunch {
    DcBlockParams p;
    long long j0 = 0, j1 = 0, j_end = 0; // complete blocks in front of the piece / behind it; blocks the piece ends in (j1 or j1 + 1)
    long long tiles = 0, ring_units = 0, units = 0;
    int tb = 0;  // blocks per tile
    int vec = 0; // in and out are on 16 bytes
};

// sample i of the filter's stream, 64 j0 <= i < t0 + n: out of the carried open block or out of the piece
template <bool SC16> __device__ __forceinline__ float2 dc_sample(const DcBlockLaunch &a, long long i) {
    if (i < a.p.t0) return a.p.open_old[i - 64 * a.j0];
    if constexpr (SC16) return sc16_widen1(static_cast<const uint32_t *>(a.p.in)[i - a.p.t0], a.p.scale);
    else return static_cast<const float2 *>(a.p.in)[i - a.p.t0];
}

// The sum of complete block k (j0 <= k < j1) by one whole wavefront, in every lane.  Steps 3 and 4 read the mirrored lane of the half
// row / row: every lane of a quad (half row) already holds the same value, so the partner's value is the one of lane ^ 4 (lane ^ 8)
template <bool SC16> __device__ __forceinline__ double2 dc_block_sum(const DcBlockLaunch &a, long long k, int lane) {
    const float2 x = dc_sample<SC16>(a, 64 * k + lane);
    double re = (double)x.x, im = (double)x.y;
    re += dpp_q<0xB1>(re);  im += dpp_q<0xB1>(im);  // quad_perm [1,0,3,2]: lane ^ 1
    re += dpp_q<0x4E>(re);  im += dpp_q<0x4E>(im);  // quad_perm [2,3,0,1]: lane ^ 2
    re += dpp_q<0x141>(re); im += dpp_q<0x141>(im); // row_half_mirror: the other quad of the half row
    re += dpp_q<0x140>(re); im += dpp_q<0x140>(im); // row_mirror: the other half of the row
    re = rows_sum16(re);    im = rows_sum16(im);    // the neighbouring row
    re = halves_sum32(re);  im = halves_sum32(im);  // the other half of the wavefront
    return make_double2(re, im);
}

// block k's sum for the state or a tile: carried (k < j0) or recomputed; lane 0 stores it
template <bool SC16> __device__ __forceinline__ void dc_sum_to(const DcBlockLaunch &a, long long k, int lane, double2 *dst) {
    if (k < a.j0) {
        if (lane == 0) *dst = a.p.ring_old[k % a.p.blocks];
    } else {
        const double2 s = dc_block_sum<SC16>(a, k, lane);
        if (lane == 0) *dst = s;
    }
}

template <bool SC16> __device__ __forceinline__ float2 dc_apply(const DcBlockLaunch &a, float2 x, long long i, long long ja, const float2 *mean) {
    const long long j = i >> 6;
    if (j == 0) return x; // block 0 has nothing in front of it
    const float2 m = mean[j - ja];
    return make_float2(x.x - m.x, x.y - m.y);
}

template <bool SC16> __global__ __launch_bounds__(256) void k_dc_block(DcBlockLaunch a) {
    __shared__ double2 s_sum[kDcMaxBlocks + kDcTileMax];
    __shared__ float2 s_mean[kDcTileMax];
    const DcBlockParams &p = a.p;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long M = p.blocks;
    for (long long u = blockIdx.x; u < a.units; u += gridDim.x) {
        if (u >= a.tiles + a.ring_units) { // the open block
            const long long i = 64 * a.j1 + threadIdx.x;
            if (i < p.t0 + p.n) p.open_new[threadIdx.x] = dc_sample<SC16>(a, i);
            continue;
        }
        if (u >= a.tiles) { // four slots of the ring
            const long long k = (a.j1 > M ? a.j1 - M : 0) + 4 * (u - a.tiles) + wave;
            if (k < a.j1) dc_sum_to<SC16>(a, k, lane, p.ring_new + k % M);
            continue;
        }
        const long long ja = a.j0 + u * a.tb, jb = ja + a.tb < a.j_end ? ja + a.tb : a.j_end;
        const long long klo = ja > M ? ja - M : 0; // the sums of [klo, jb - 1): every one a complete block
        for (long long k = klo + wave; k < jb - 1; k += 4) dc_sum_to<SC16>(a, k, lane, s_sum + (k - klo));
        __syncthreads();
        if (wave == 0 && ja + lane < jb) {
            const long long j = ja + lane, lo = j > M ? j - M : 0;
            float2 m = make_float2(0.f, 0.f);
            if (lo < j) {
                double2 acc = s_sum[lo - klo];
                for (long long k = lo + 1; k < j; ++k) {
                    const double2 b = s_sum[k - klo];
                    acc.x += b.x;
                    acc.y += b.y;
                }
                const double d = 64.0 * (double)(j - lo);
                m = make_float2((float)(acc.x / d), (float)(acc.y / d));
            }
            s_mean[lane] = m;
        }
        __syncthreads();
        // the tile's samples that lie in the piece, as indices into the piece
        const long long e_lo = 64 * ja > p.t0 ? 64 * ja - p.t0 : 0, e_hi = (64 * jb < p.t0 + p.n ? 64 * jb : p.t0 + p.n) - p.t0;
        for (long long e0 = 4 * ((e_lo >> 2) + threadIdx.x); e0 < e_hi; e0 += 4 * 256) {
            if (a.vec && e0 >= e_lo && e0 + 4 <= e_hi) {
                float2 x[4];
                if constexpr (SC16) {
                    const uint4 d = *reinterpret_cast<const uint4 *>(static_cast<const uint32_t *>(p.in) + e0);
                    x[0] = sc16_widen1(d.x, p.scale); x[1] = sc16_widen1(d.y, p.scale);
                    x[2] = sc16_widen1(d.z, p.scale); x[3] = sc16_widen1(d.w, p.scale);
                } else {
                    const float4 *src = reinterpret_cast<const float4 *>(static_cast<const float2 *>(p.in) + e0);
                    const float4 v0 = src[0], v1 = src[1];
                    x[0] = make_float2(v0.x, v0.y); x[1] = make_float2(v0.z, v0.w);
                    x[2] = make_float2(v1.x, v1.y); x[3] = make_float2(v1.z, v1.w);
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) x[q] = dc_apply<SC16>(a, x[q], p.t0 + e0 + q, ja, s_mean);
                float4 *o = reinterpret_cast<float4 *>(p.out + e0);
                o[0] = make_float4(x[0].x, x[0].y, x[1].x, x[1].y);
                o[1] = make_float4(x[2].x, x[2].y, x[3].x, x[3].y);
            } else {
                for (long long e = e0 > e_lo ? e0 : e_lo; e < e0 + 4 && e < e_hi; ++e)
                    p.out[e] = dc_apply<SC16>(a, dc_sample<SC16>(a, p.t0 + e), p.t0 + e, ja, s_mean);
            }
        }
        __syncthreads(); // the next tile of this workgroup overwrites s_sum and s_mean
    }
}

hipError_t run_dc_block(const DcBlockParams &p, bool sc16, int num_cu, hipStream_t st) {
    if (p.n < 0 || p.t0 < 0 || p.blocks < 1 || p.blocks > kDcMaxBlocks) return hipErrorInvalidValue;
    if (p.n == 0) return hipSuccess;
    if (!p.in || !p.out || !p.ring_old || !p.ring_new || !p.open_old || !p.open_new) return hipErrorInvalidValue;
    DcBlockLaunch a;
    a.p = p;
    a.j0 = p.t0 / 64;
    a.j1 = (p.t0 + p.n) / 64;
    a.j_end = (p.t0 + p.n + 63) / 64;
    a.tb = p.blocks > 16 ? kDcTileMax : 16;
    a.tiles = (a.j_end - a.j0 + a.tb - 1) / a.tb;
    const long long live = a.j1 < p.blocks ? a.j1 : p.blocks; // the ring slots in use behind the piece
    a.ring_units = a.j1 > a.j0 ? (live + 3) / 4 : 0;
    a.units = a.tiles + a.ring_units + ((p.t0 + p.n) % 64 ? 1 : 0);
    a.vec = ((reinterpret_cast<uintptr_t>(p.in) | reinterpret_cast<uintptr_t>(p.out)) & 15) == 0;
    const dim3 grid((unsigned)persistent_grid(a.units, (long long)num_cu * 8, tuning_or_default(p.tune)));
    trace_add(p.trace, sc16 ? "k_dc_block<sc16>" : "k_dc_block<fc32>");
    if (sc16) hipLaunchKernelGGL(k_dc_block<true>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_dc_block<false>, grid, dim3(256), 0, st, a);
    return hipGetLastError();
}

} // namespace ofdm
