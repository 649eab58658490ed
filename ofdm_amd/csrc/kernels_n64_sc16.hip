// kernels_n64_sc16.hip -- EXT-9: k_demod64_sc16, the N = 64 RX demod of kernels_n64.hip fed with sc16 samples (interleaved
// little-endian int16 I/Q, 4 bytes a sample).
//
// k_demod64's mapping, unchanged: one 64-lane wavefront owns 8 consecutive symbols, lane (s, t) owns points t + 8 m, no workgroup
// barrier.  What differs is the fetch: 8 x global_load_dword with immediate offsets 32 bytes apart from a scalar base, where the fc32
// kernel issues 8 x dwordx2 64 bytes apart.  A symbol is 320 bytes (2.5 cache lines), its 64-byte cyclic prefix half a line: the eight
// lanes of a symbol read 32 contiguous bytes per load, and the eight loads together cover the symbol's 256 data bytes once.  Each dword
// is split into its sign-extended halves, converted and multiplied by `scale` -- one rounded f32 product per component, issued as its
// own v_mul_f32 so that it cannot be contracted into the first butterfly's additions (include/ofdm_hip.h, "sc16") -- and from there on
// the body is k_demod64's, operation for operation: the bytes are those of k_demod64 on the widened samples.
// The body is a copy, not a shared __device__ function: k_demod64's device code must stay what it is (tools/isa_identity.py), and
// the profiling exits and the store-policy probe of the fc32 kernel are not carried over.
// Roofline: HBM -- 320 algorithmic bytes read per symbol (256 of them data; the prefix shares lines with data) + packed bytes written.
#include "device_common.hpp"
#include "kernels.hpp"
#include <type_traits>

namespace ofdm {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) f32x2 *lds_cf_ptr;
typedef __attribute__((address_space(3))) unsigned *lds_u32_ptr;


template <int BPS, bool GUARD, bool HK, int BURST = 1>
__global__ __launch_bounds__(256, 4) void k_demod64_sc16(Fast64Sc16Params p) {
    constexpr int S = 80, CP = 16;
    constexpr int ND = GUARD ? 48 : 64;          // data carriers per symbol
    constexpr int REGION_DW = ND * BPS / 4;      // packed output of 8 symbols, in dwords
    constexpr int SLAB = 8 * 72;                 // 8 symbols x (64 + 8 pad) points

    __shared__ cf slab_all[4 * SLAB];
    __shared__ __align__(16) unsigned img_all[4 * BURST * REGION_DW];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int s = lane >> 3, t = lane & 7;
    cf *buf = slab_all + wave * SLAB + s * 72;
    unsigned *img0 = img_all + wave * BURST * REGION_DW;

    // loop-invariant per-lane constants
    cf w[7];
#pragma unroll
    for (int r = 1; r < 8; ++r) w[r - 1] = p.tw[r * t];
    cf g[8];
    if (HK) {
#pragma unroll
        for (int m = 0; m < 8; ++m) { // 1 / H
            cf h = p.hk[t + 8 * m];
            float ns = h.x * h.x + h.y * h.y;
            g[m] = make_float2(h.x / ns, -h.y / ns);
        }
    }
    unsigned wa[8], ra[8], fa[8], fs[8]; // LDS byte addresses of the transpose and of every field's dword; fs: shift, 0xFFFFFFFF = not a data bin
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        wa[r] = pinned(lds_addr(buf + (swz(8 * t) ^ r)));
        ra[r] = pinned(lds_addr(buf + 8 * r + (t ^ r)));
        const int c = t + 8 * r;
        const int q = GUARD ? data_classes_below64(c) : c;
        const int bo = (s * ND + q) * BPS;
        const bool data = carrier_class64(c, GUARD) == 0;
        fa[r] = pinned(lds_addr(img0 + (bo >> 5)));
        fs[r] = pinned(data ? (unsigned)(bo & 31) : 0xFFFFFFFFu);
    }
    const int lane_off = s * S + t; // sample offset of this lane inside the 8-symbol group

    auto group = [&](long long f, int kk, unsigned img_off) {
        const uint32_t *src = p.in16 + f * p.frame_stride + (long long)(p.first_symbol + kk * 8) * S + CP + lane_off;
        unsigned d[8];
#pragma unroll
        for (int m = 0; m < 8; ++m) d[m] = src[8 * m];
        cf v[8];
#pragma unroll
        for (int m = 0; m < 8; ++m) v[m] = sc16_widen1(d[m], p.scale);
        bfly8<false>(v);
#pragma unroll
        for (int r = 0; r < 8; ++r) *(lds_cf_ptr)(unsigned long)wa[r] = f32x2{v[r].x, v[r].y};
#pragma unroll
        for (int m = 0; m < 8; ++m) { const f32x2 q = *(lds_cf_ptr)(unsigned long)ra[m]; v[m] = make_float2(q.x, q.y); }
#pragma unroll
        for (int r = 1; r < 8; ++r) v[r] = cmul(v[r], w[r - 1]);
        bfly8<false>(v);
        // v[m] = X[t + 8m]
        if (HK) {
#pragma unroll
            for (int m = 0; m < 8; ++m) v[m] = cmul(v[m], g[m]);
        }
        cf rot = make_float2(1.f, 0.f);
        if (GUARD) { // mean of the 4 pilot angles (bins 6, 25, 39, 58), in turns, as k_demod64
            cf pv = make_float2(1.f, 0.f);
            pv = (t == 6) ? v[0] : pv;
            pv = (t == 1) ? v[3] : pv;
            pv = (t == 7) ? v[4] : pv;
            pv = (t == 2) ? v[7] : pv;
            const float turns = sum8_lanes(__ocml_atan2pi_f32(pv.y, pv.x)) * 0.125f;
            rot = make_float2(__builtin_amdgcn_cosf(turns), -__builtin_amdgcn_sinf(turns));
        }
        // clear the packed image, OR every field in
        unsigned *img = reinterpret_cast<unsigned *>(reinterpret_cast<unsigned char *>(img0) + img_off);
        for (int i = lane; i < REGION_DW; i += 64) img[i] = 0u;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const bool all_data = !GUARD || m == 1 || m == 2 || m == 5 || m == 6;
            if (all_data || fs[m] != 0xFFFFFFFFu) {
                const unsigned idx = GUARD ? demap_point_rot(v[m], rot, BPS) : demap_point(v[m], BPS);
                const lds_u32_ptr wd = (lds_u32_ptr)(unsigned long)(fa[m] + img_off);
                __hip_atomic_fetch_or(wd, idx << fs[m], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (BPS > 1 && (32 % BPS) != 0) { // a field may straddle two dwords (only for 6-bit fields)
                    if (fs[m] + BPS > 32) __hip_atomic_fetch_or(wd + 1, idx >> (32 - fs[m]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
    };
    auto store_image = [&](unsigned *dst, int ndw) { // ndw dwords of this wave's LDS image -> global
        if ((REGION_DW % 4) == 0 && p.wide_stores) // 16 bytes per lane
            for (int i = lane; i < ndw / 4; i += 64) reinterpret_cast<uint4 *>(dst)[i] = reinterpret_cast<const uint4 *>(img0)[i];
        else for (int i = lane; i < ndw; i += 64) dst[i] = img0[i];
    };

    if (BURST > 1) {
        // wave-uniform: burst j of this wave = groups [BURST j, BURST (j + 1)); one 64-bit division per BURST groups
        const long long n_bursts = p.n_groups / BURST; // the launcher guarantees divisibility and a contiguous output
        for (long long j = (long long)blockIdx.x * 4 + wave; j < n_bursts; j += p.stride_groups) {
            const long long g0 = j * BURST;
            long long f = g0 / p.groups_per_frame;
            int kk = (int)(g0 - f * p.groups_per_frame);
#pragma nounroll
            for (int b = 0; b < BURST; ++b) {
                group(f, kk, (unsigned)(b * REGION_DW * 4));
                if (++kk == p.groups_per_frame) { kk = 0; ++f; }
            }
            store_image(reinterpret_cast<unsigned *>(p.out + g0 * (long long)(REGION_DW * 4)), BURST * REGION_DW);
        }
        return;
    }

    // wave-uniform iteration state (no division in the loop: the host supplies the per-step increments)
    long long f = p.f0 + (long long)blockIdx.x * p.blk_df + wave * p.wave_df;
    int kk = p.k0 + (int)((blockIdx.x * (long long)p.blk_dk + wave * p.wave_dk));
    f += kk / p.groups_per_frame;
    kk %= p.groups_per_frame;
    for (long long g_idx = (long long)blockIdx.x * 4 + wave; g_idx < p.n_groups; g_idx += p.stride_groups) {
        group(f, kk, 0u);
        store_image(reinterpret_cast<unsigned *>(p.out + f * p.out_stride + (long long)kk * 8 * (ND * BPS / 8)), REGION_DW);
        f += p.step_df;
        kk += p.step_dk;
        if (kk >= p.groups_per_frame) { kk -= p.groups_per_frame; f += 1; }
    }
}

// launch_demod64's rules (kernels_n64.hip): store width, burst length, persistent grid, index increments
template <int BPS, bool GUARD, bool HK> static hipError_t launch_demod64_sc16(Fast64Sc16Params p, hipStream_t st, int num_cu, const Tuning &tu, Trace *trace) {
    constexpr int region_bytes = (GUARD ? 48 : 64) * BPS;
    p.wide_stores = !tu.demod64_narrow_stores && region_bytes % 16 == 0 && (reinterpret_cast<uintptr_t>(p.out) & 15) == 0 && (p.out_stride & 15) == 0;
    const bool burst = BPS == 6 && GUARD && !HK && tu.demod64_burst >= 4 && p.wide_stores && p.n_groups % 4 == 0 &&
                       p.out_stride == (long long)p.groups_per_frame * region_bytes && (reinterpret_cast<uintptr_t>(p.out) & 127) == 0;
    const int burst_cap = tu.demod64_burst;
    const int bl = !burst ? 1 : (burst_cap >= 16 && p.n_groups % 16 == 0) ? 16 : (burst_cap >= 8 && p.n_groups % 8 == 0) ? 8 : 4;
    auto kernel = !burst ? k_demod64_sc16<BPS, GUARD, HK, 1> : bl == 16 ? k_demod64_sc16<6, true, false, 16> : bl == 8 ? k_demod64_sc16<6, true, false, 8> : k_demod64_sc16<6, true, false, 4>;
    const long long units = burst ? p.n_groups / bl : p.n_groups;
    const int knob = tu.demod64_wg_per_cu;
    const int per_cu = knob > 0 ? knob : (resident_blocks(kernel, 256) >= 4 ? 8 : 2 * resident_blocks(kernel, 256));
    const int grid = (int)persistent_grid((units + 3) / 4, (long long)num_cu * per_cu, tu); // a workgroup = four waves, a unit each
    trace_add(trace, !burst ? "k_demod64_sc16" : bl == 16 ? "k_demod64_sc16<burst16>" : bl == 8 ? "k_demod64_sc16<burst8>" : "k_demod64_sc16<burst4>");
    p.stride_groups = (long long)grid * 4;
    const int gpf = p.groups_per_frame;
    p.f0 = 0; p.k0 = 0;
    p.blk_df = 4 / gpf; p.blk_dk = 4 % gpf;
    p.wave_df = 0; p.wave_dk = 1;
    p.step_df = p.stride_groups / gpf; p.step_dk = (int)(p.stride_groups % gpf);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, st, p);
    return hipGetLastError();
}

hipError_t run_demod64_sc16(const SymParams &sp, const uint32_t *in16, float scale, hipStream_t st, int num_cu) {
    if (sp.offset || sp.f_delta || sp.nsym_frame || sp.soft) return hipErrorNotSupported;
    if (sp.syms_per_frame <= 0 || (sp.syms_per_frame & 7) != 0) return hipErrorNotSupported;
    if (sp.hk && sp.hk_stride != 0) return hipErrorNotSupported;
    if ((long long)(sp.first_symbol + sp.syms_per_frame) * 80 > sp.frame_len) return hipErrorNotSupported; // no tail padding
    if ((reinterpret_cast<uintptr_t>(sp.out_bytes) & 3) || (sp.out_stride & 3)) return hipErrorNotSupported;
    if (reinterpret_cast<uintptr_t>(in16) & 3) return hipErrorNotSupported;
    Fast64Sc16Params p;
    p.in16 = in16; p.scale = scale; p.frame_stride = sp.frame_stride; p.first_symbol = sp.first_symbol;
    p.hk = sp.hk; p.tw = sp.tw; p.out = sp.out_bytes; p.out_stride = sp.out_stride;
    p.groups_per_frame = sp.syms_per_frame / 8;
    p.n_groups = sp.n_frames * (long long)p.groups_per_frame;
    if (p.n_groups <= 0) return hipSuccess;
    const Tuning &tu = tuning_or_default(sp.tune);
    return with_bps(sp.bps, [&](auto B) { return with_bool(sp.guard != 0, [&](auto G) { return with_bool(p.hk != nullptr, [&](auto H) {
        return launch_demod64_sc16<decltype(B)::value, decltype(G)::value, decltype(H)::value>(p, st, num_cu, tu, sp.trace); }); }); });
}

} // namespace ofdm
