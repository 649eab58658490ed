// kernels_sc16.hip -- EXT-9: sc16 (interleaved little-endian int16 I/Q, UHD's wire format) <-> fc32.  Definition: include/ofdm_hip.h;
// numpy restatement: tests/sc16_ref.py.
//   k_sc16_widen    x = (float)v * scale per component: 4 B in, 8 B out a sample
//   k_sc16_narrow   q = clamp(rint(x * scale), +-32767), NaN -> 0, clipped components counted per row: 8 B in, 4 B out a sample
// Both are streaming passes bound by HBM: no LDS, no workspace, a persistent grid over tiles of 1024 samples (256 threads x 4 samples).
// A thread moves its four samples with 16-byte accesses (widen: one load, two stores; narrow: two loads, one store) when base
// addresses and strides allow it for EVERY row, and sample by sample otherwise or in a row's ragged tail.
// The product is issued as its own v_mul_f32 (sc16_mul, device_common.hpp).
#include "device_common.hpp"
#include "kernels.hpp"
#include <cmath>

namespace ofdm {

constexpr int kSc16Tile = 1024; // samples per workgroup step

// (sc16_narrow1 / sc16_narrow2, the rule of one component and of one sample, are in device_common.hpp: k_txframe64_sc16 uses them too)
struct Sc16Launch {
    Sc16Params p;
    long long units = 0, tiles_per_row = 1;
    int vec = 0; // 16-byte accesses are aligned in every row
};

__global__ __launch_bounds__(256) void k_sc16_widen(Sc16Launch a) {
    const Sc16Params &p = a.p;
    for (long long u = blockIdx.x; u < a.units; u += gridDim.x) {
        const long long row = u / a.tiles_per_row;
        const long long i0 = (u - row * a.tiles_per_row) * kSc16Tile + 4 * (long long)threadIdx.x;
        const uint32_t *src = p.sc_in + row * p.in_stride;
        float2 *dst = p.fc_out + row * p.out_stride;
        if (a.vec && i0 + 4 <= p.frame_len) {
            const uint4 d = *reinterpret_cast<const uint4 *>(src + i0);
            const float2 s0 = sc16_widen1(d.x, p.scale), s1 = sc16_widen1(d.y, p.scale);
            const float2 s2 = sc16_widen1(d.z, p.scale), s3 = sc16_widen1(d.w, p.scale);
            float4 *o = reinterpret_cast<float4 *>(dst + i0);
            o[0] = make_float4(s0.x, s0.y, s1.x, s1.y);
            o[1] = make_float4(s2.x, s2.y, s3.x, s3.y);
        } else {
            for (long long i = i0; i < i0 + 4 && i < p.frame_len; ++i) dst[i] = sc16_widen1(src[i], p.scale);
        }
    }
}

__global__ __launch_bounds__(256) void k_sc16_narrow(Sc16Launch a) {
    const Sc16Params &p = a.p;
    for (long long u = blockIdx.x; u < a.units; u += gridDim.x) {
        const long long row = u / a.tiles_per_row;
        const long long i0 = (u - row * a.tiles_per_row) * kSc16Tile + 4 * (long long)threadIdx.x;
        const float2 *src = p.fc_in + row * p.in_stride;
        uint32_t *dst = p.sc_out + row * p.out_stride;
        int clipped = 0;
        if (a.vec && i0 + 4 <= p.frame_len) {
            const float4 x0 = reinterpret_cast<const float4 *>(src + i0)[0], x1 = reinterpret_cast<const float4 *>(src + i0)[1];
            uint4 d;
            d.x = sc16_narrow2(make_float2(x0.x, x0.y), p.scale, &clipped);
            d.y = sc16_narrow2(make_float2(x0.z, x0.w), p.scale, &clipped);
            d.z = sc16_narrow2(make_float2(x1.x, x1.y), p.scale, &clipped);
            d.w = sc16_narrow2(make_float2(x1.z, x1.w), p.scale, &clipped);
            *reinterpret_cast<uint4 *>(dst + i0) = d;
        } else {
            for (long long i = i0; i < i0 + 4 && i < p.frame_len; ++i) dst[i] = sc16_narrow2(src[i], p.scale, &clipped);
        }
        if (p.clipped) { // an integer count: any order of the additions gives the same number
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) clipped += __shfl_xor(clipped, m, 64);
            if ((threadIdx.x & 63) == 0 && clipped) atomicAdd(p.clipped + row, clipped);
        }
    }
}

static Sc16Launch sc16_plan(const Sc16Params &p, uintptr_t sc_base, uintptr_t fc_base, long long sc_stride, long long fc_stride, bool merge) {
    Sc16Launch a;
    a.p = p;
    // rows back to back on both sides are one long row (never for a narrow that counts per row)
    if (merge && p.in_stride == p.frame_len && p.out_stride == p.frame_len) {
        a.p.frame_len = p.n_frames * p.frame_len;
        a.p.n_frames = 1;
        a.p.in_stride = a.p.out_stride = a.p.frame_len;
    }
    const bool one = a.p.n_frames == 1;
    a.vec = (sc_base & 15) == 0 && (fc_base & 15) == 0 && (one || ((sc_stride & 3) == 0 && (fc_stride & 1) == 0));
    a.tiles_per_row = (a.p.frame_len + kSc16Tile - 1) / kSc16Tile;
    a.units = a.p.n_frames * a.tiles_per_row;
    return a;
}

hipError_t run_sc16_widen(const Sc16Params &p, int num_cu, hipStream_t st) {
    if (p.n_frames <= 0 || p.frame_len <= 0) return hipSuccess;
    const Sc16Launch a = sc16_plan(p, reinterpret_cast<uintptr_t>(p.sc_in), reinterpret_cast<uintptr_t>(p.fc_out), p.in_stride, p.out_stride, true);
    const dim3 grid((unsigned)persistent_grid(a.units, (long long)num_cu * 8, tuning_or_default(p.tune)));
    trace_add(p.trace, "k_sc16_widen");
    hipLaunchKernelGGL(k_sc16_widen, grid, dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t run_sc16_narrow(const Sc16Params &p, int num_cu, hipStream_t st) {
    if (p.n_frames <= 0) return hipSuccess;
    if (p.clipped) {
        const hipError_t e = hipMemsetAsync(p.clipped, 0, sizeof(int32_t) * (size_t)p.n_frames, st);
        if (e != hipSuccess) return e;
    }
    if (p.frame_len <= 0) return hipSuccess;
    const Sc16Launch a = sc16_plan(p, reinterpret_cast<uintptr_t>(p.sc_out), reinterpret_cast<uintptr_t>(p.fc_in), p.out_stride, p.in_stride, !p.clipped);
    const dim3 grid((unsigned)persistent_grid(a.units, (long long)num_cu * 8, tuning_or_default(p.tune)));
    trace_add(p.trace, "k_sc16_narrow");
    hipLaunchKernelGGL(k_sc16_narrow, grid, dim3(256), 0, st, a);
    return hipGetLastError();
}

// ---- the definition in C (ofdm_sc16_widen / ofdm_sc16_narrow): no device
void sc16_widen_host(const int16_t *in, long long n, float scale, float *out) {
    for (long long i = 0; i < 2 * n; ++i) out[i] = (float)in[i] * scale;
}
long long sc16_narrow_host(const float *in, long long n, float scale, int16_t *out) {
    long long clipped = 0;
    for (long long i = 0; i < 2 * n; ++i) {
        const float r = std::nearbyint(in[i] * scale); // the default rounding mode: to nearest, ties to even
        if (!(std::fabs(r) <= 32767.f)) ++clipped;
        out[i] = (int16_t)(r != r ? 0.f : std::fmin(std::fmax(r, -32767.f), 32767.f));
    }
    return clipped;
}

} // namespace ofdm
