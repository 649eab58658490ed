// kernels_n64.hip -- the shape-specialised N = 64 kernels of the hot path (everything without a kernel of its own is the generic k_sym):
//   k_demod64      N = 64 RX demod for regular streams (BASELINE config 2, the headline)      -- described below
//   k_rxframe64    N = 64 per-frame receive body after timing (config 3): channel estimate + demod [+ finish]
//   k_txframe64    N = 64 encode: frame built in LDS, one HBM pass
//   (k_rxframe1024, the N = 1024 per-frame receive body of config 4, lives in kernels_rx1024.hip; k_demod4096 / k_tx4096 /
//    k_txframe4096, N = 4096 as 64 x 64, in kernels_n4096.hip; k_demod64_sc16, k_demod64 fed with int16 samples, in kernels_n64_sc16.hip)
//
// k_demod64: CP strip + FFT64 + [equalise] + pilot phase + hard demap + LSB-first bit packing, for regularly spaced,
// HBM-resident symbols.
//
// Wave-centric: one 64-lane wavefront owns 8 consecutive OFDM symbols (8 lanes x 8 points each) per iteration and
// never meets a workgroup barrier.  Per iteration and lane:
//   8 x global_load_dwordx2 with immediate offsets (the 128-byte cyclic prefix of each 640-byte symbol is a whole,
//     aligned cache line and is never fetched), scalar base address, no integer division anywhere;
//   radix-8 butterfly -> XOR-swizzled LDS slab -> radix-8 butterfly (7 loop-invariant twiddles in registers);
//   pilot phase: atan2 on the 4 pilot lanes, 3 DPP adds inside the 8-lane group, one sincos;
//   hard decisions; bit fields OR-ed into the wave's packed output image in LDS (ds_or_b32), then the image is
//   stored with unit-stride dword stores (36 B per symbol for 64-QAM with guard bands).
// Roofline: HBM -- 640 algorithmic bytes read per symbol (512 actually fetched) + packed bytes written.
#include "device_common.hpp"
#include "kernels.hpp"
#include <type_traits>
#include <stdlib.h>

namespace ofdm {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) f32x2 *lds_cf_ptr; // LDS pointer built from a 32-bit offset held in a VGPR
typedef __attribute__((address_space(3))) unsigned *lds_u32_ptr;
// BURST (4, 8 or 16): a wavefront takes BURST consecutive 8-symbol groups per step and stores their packed images together -- for the
// 288-byte images of 64-QAM with guard bands, 4 groups = 1152 bytes = nine WHOLE 128-byte lines (one group's image starts at
// a multiple of 288 bytes: 2.25 lines, shared with the neighbours).  Needs a contiguous output (rows back to back).
template <int BPS, bool GUARD, bool HK, int BURST = 1>
__global__ __launch_bounds__(256, 4) void k_demod64(Fast64Params p) {
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
        for (int m = 0; m < 8; ++m) { // 1 / H  (equalise: Y /= H, src/receiver.rs:68-70)
            cf h = p.hk[t + 8 * m];
            float ns = h.x * h.x + h.y * h.y;
            g[m] = make_float2(h.x / ns, -h.y / ns);
        }
    }
    // LDS byte addresses of the transpose (write: swz(8t + r) = 8t + (r ^ t); read: swz(t + 8m) = 8m + (t ^ m)) and of every
    // field's dword in the packed image, with the field's shift: 8 + 8 + 8 + 8 registers instead of ~5 integer instructions
    // per access and iteration
    unsigned wa[8], ra[8], fa[8], fs[8]; // fs: bit shift inside the dword, 0xFFFFFFFF = not a data bin
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

    // one 8-symbol group: CP strip + FFT64 + [equalise] + pilot phase + demap + packing into the LDS image at byte offset img_off
    auto group = [&](long long f, int kk, unsigned img_off) {
        const cf *src = p.in + f * p.frame_stride + (long long)(p.first_symbol + kk * 8) * S + CP + lane_off;
        cf v[8];
#pragma unroll
        for (int m = 0; m < 8; ++m) v[m] = src[8 * m];
        bfly8<false>(v);
        if (kProfile && p.debug == 3) { // profiling aid: loads + one butterfly
            float acc = 0.f;
#pragma unroll
            for (int m = 0; m < 8; ++m) acc += v[m].x + v[m].y;
            if (acc == 12345.678f) p.out[0] = 1;
            return;
        }
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
        if (GUARD) {
            // decode_block (src/receiver.rs:106-145): mean of the 4 pilot angles, rotate data points by -phase
            // pilots sit at bins 6, 25, 39, 58 = lanes t = 6 (m 0), 1 (m 3), 7 (m 4), 2 (m 7); the other lanes
            // feed (1, 0) -> angle 0, so ONE atan2 evaluation serves the whole wave
            cf pv = make_float2(1.f, 0.f);
            pv = (t == 6) ? v[0] : pv;
            pv = (t == 1) ? v[3] : pv;
            pv = (t == 7) ? v[4] : pv;
            pv = (t == 2) ? v[7] : pv;
            // mean angle in TURNS (sum of the four atan2pi values / 8), then the hardware sine / cosine, which take turns:
            // max abs error 1.3e-7 over [-pi, pi] on gfx950 (tools/lab/trig_probe.cpp; sincospif: 5e-8) for 2 instructions instead of ~35
            const float turns = sum8_lanes(__ocml_atan2pi_f32(pv.y, pv.x)) * 0.125f;
            rot = make_float2(__builtin_amdgcn_cosf(turns), -__builtin_amdgcn_sinf(turns)); // applied inside the demapper (demap_point_rot)
        }
        if (kProfile && p.debug == 2) { // profiling aid: everything but the packing and the stores
            float acc = 0.f;
#pragma unroll
            for (int m = 0; m < 8; ++m) acc += v[m].x + v[m].y;
            if (acc == 12345.678f) p.out[0] = 1;
            return;
        }
        // clear the packed image, OR every field in
        unsigned *img = reinterpret_cast<unsigned *>(reinterpret_cast<unsigned char *>(img0) + img_off);
        for (int i = lane; i < REGION_DW; i += 64) img[i] = 0u;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            // bins t + 8 m with m in {1, 2, 5, 6} are data carriers for every lane (the nulls and pilots sit in rows 0, 3, 4, 7):
            // no per-lane test, no exec-mask juggling for half of the fields
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
        if (kProfile && (p.debug == 1 || p.debug == 2 || p.debug == 3)) { if (img0[lane] == 0x12345678u) dst[0] = 1u; return; } // profiling aid: no stores
        if (kProfile && p.debug == 4) dst = reinterpret_cast<unsigned *>(p.out) + (blockIdx.x & 255) * 4 * BURST * REGION_DW + wave * BURST * REGION_DW; // L2-resident window
        if (kProfile && p.debug == 5) { for (int i = lane; i < ndw; i += 64) __builtin_nontemporal_store(img0[i], dst + i); return; }
        if ((REGION_DW % 4) == 0 && p.wide_stores) { // 16 bytes per lane
            if (p.store_policy) {   // lab key demod64_store_policy: 1 = nt, 2 = sc1, 3 = sc0 sc1 on the image stores (the output-buffer populations)
                typedef unsigned v4u __attribute__((ext_vector_type(4)));
                for (int i = lane; i < ndw / 4; i += 64) {
                    const v4u val = reinterpret_cast<const v4u *>(img0)[i];
                    uint4 *a = reinterpret_cast<uint4 *>(dst) + i;
                    if (p.store_policy == 1) asm volatile("global_store_dwordx4 %0, %1, off nt" ::"v"(a), "v"(val) : "memory");
                    else if (p.store_policy == 2) asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(a), "v"(val) : "memory");
                    else asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" ::"v"(a), "v"(val) : "memory");
                }
                return;
            }
            for (int i = lane; i < ndw / 4; i += 64) reinterpret_cast<uint4 *>(dst)[i] = reinterpret_cast<const uint4 *>(img0)[i];
        } else for (int i = lane; i < ndw; i += 64) dst[i] = img0[i];
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
    // normalise kk into [0, groups_per_frame)
    f += kk / p.groups_per_frame;
    kk %= p.groups_per_frame;
    for (long long g_idx = (long long)blockIdx.x * 4 + wave; g_idx < p.n_groups; g_idx += p.stride_groups) {
        group(f, kk, 0u);
        store_image(reinterpret_cast<unsigned *>(p.out + f * p.out_stride + (long long)kk * 8 * (ND * BPS / 8)), REGION_DW);
        // advance (wave-uniform)
        f += p.step_df;
        kk += p.step_dk;
        if (kk >= p.groups_per_frame) { kk -= p.groups_per_frame; f += 1; }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// k_rxframe64: the per-frame RX body for N = 64 after timing (BASELINE config 3): for every frame, one wavefront does
//   estimate_channel (src/receiver.rs:212-229) on the 5 training blocks  -> 1/H kept in registers
//   then per group of 8 data symbols: CFO derotation (receiver.rs:44-50, phase reduced in f64), CP strip + FFT64
//   (receiver.rs:99-104), equalise (receiver.rs:68-70), pilot phase (receiver.rs:106-145), hard demap + LSB-first packing
//   (receiver.rs:147-190).  Frames may start at any sample offset (8-byte aligned loads), samples at or beyond
//   frame_len read as zero (pad_chunk).  No workgroup barrier: the 4 waves of a workgroup own 4 different frames.
//   (Round 2 measured a variant with the next group's / next frame's samples prefetched into registers: 242 VGPRs, two
//   waves per SIMD, 1.12 ms per 262 144 config-3 frames against 0.94-1.14 ms for this one: no gain, not kept.)
struct RxFrame64Params {
    const float2 *in;
    long long n_frames, frame_stride, frame_len;
    const int32_t *offset;
    const double *f_delta;
    const int32_t *nsym;       // live data symbols per frame (0 = skip)
    const float2 *tw, *inv_training;
    unsigned char *out;        // raw decoded bytes, nsym * bytes_per_symbol per frame
    long long out_stride;
    float2 *hk;                // optional: channel estimate per frame (64 bins)
    // optional fused "finish" (length header parse + truncate, src/receiver.rs:85-95; no outer code): when final_out is set the
    // decoded bytes go straight to their final place (raw byte 16 + i -> final byte i, i < length) and `out` is unused
    unsigned char *final_out;
    long long final_stride;
    int32_t *final_len;
    const int32_t *frame_list;   // optional: only these frames (count on the device)
    const int32_t *frame_count;
    int32_t *cut_list;           // MODE 0: frames whose capture ends inside the frame are appended here (count at cut_count) for the MODE 1 launch
    int32_t *cut_count;
};

__device__ __forceinline__ cf lane_xor_sum(cf v) { // sum over the 8 symbol slots: lanes with equal (lane & 7)
    v.x += dpp_f<0x128>(v.x); v.y += dpp_f<0x128>(v.y);          // row_ror:8  : lane ^ 8
    v.x += __shfl_xor(v.x, 16, 64); v.y += __shfl_xor(v.y, 16, 64);
    v.x += __shfl_xor(v.x, 32, 64); v.y += __shfl_xor(v.y, 32, 64);
    return v;
}

// MODE (round 4): the body exists twice -- for frames that lie wholly inside their capture, and for captures that END inside the
// frame (zero-filled tail, pad_chunk) -- and with both in one kernel the register budget is the larger one's: 168 VGPRs, three
// waves per SIMD.  MODE 0 holds only the common body (126 VGPRs with guard bands: FOUR waves per SIMD -- the kernel is VALU-issue
// bound and three waves cannot fill the pipe) and appends the frames it has to leave to a device-side list; MODE 1
// holds only the cut body and runs over that list (normally empty: microseconds); MODE 2 is the round-3 kernel with both bodies,
// for callers that bring their own frame list (the one-pass kernel's slow list).
template <int BPS, bool GUARD, int MODE>
__global__ __launch_bounds__(256, (MODE == 0 && GUARD) ? 4 : 3) void k_rxframe64(RxFrame64Params p) {
    constexpr int S = 80, CP = 16;
    constexpr int ND = GUARD ? 48 : 64;
    constexpr int SYM_BYTES = ND * BPS / 8;   // a multiple of 4, or 6 (BPSK with guard bands: the reference's default frame): eight symbols are whole dwords either way
    constexpr int REGION_DW = ND * BPS / 4;   // 8 symbols
    constexpr int SLAB = 8 * 72;
    __shared__ cf slab_all[4 * SLAB];
    __shared__ cf ginv_all[4 * 64];           // 1 / H per wavefront, read at use (16 fewer live registers than a register copy)
    __shared__ unsigned img_all[4 * REGION_DW];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int s = lane >> 3, t = lane & 7;
    cf *buf = slab_all + wave * SLAB + s * 72;
    unsigned *img = img_all + wave * REGION_DW;

    // Lane constants that k_demod64 keeps in registers live in LDS here (22 VGPRs): with a second set of sample registers for the
    // next group's prefetch the kernel would otherwise spill at three waves per SIMD, and a spill reload waits for vmcnt(0),
    // i.e. for the prefetch.  twl[m] = W64^m (the stage twiddles W64^(r t) and the one-point-per-lane transform's twiddles: as
    // global loads their six loop-invariant 64-bit addresses are hoisted by the compiler and one of them spills);
    // bofftab[m * 64 + lane] = bit offset of bin t + 8 m, -1 = not data.
    __shared__ cf twl[64];
    __shared__ int bofftab[8 * 64];
    if (threadIdx.x < 64) twl[threadIdx.x] = p.tw[threadIdx.x];
    if (wave == 0) {
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int c = t + 8 * m;
            const int q = GUARD ? data_classes_below64(c) : c;
            bofftab[m * 64 + lane] = (carrier_class64(c, GUARD) == 0) ? (s * ND + q) * BPS : -1;
        }
    }
    __shared__ int cutbuf[4][1 + 16];         // MODE 0: per wavefront, the cut frames not yet on the global list (batched: one atomic per 16)
    if (MODE == 0 && lane == 0) cutbuf[wave][0] = 0;
    __syncthreads();
    const int wr = swz(8 * t);
    auto cut_flush = [&]() { // lane 0 only; this wavefront's own slots: no other wavefront reads or writes them
        const int m = cutbuf[wave][0];
        if (m > 0) {
            const int base = atomicAdd(p.cut_count, m);
            for (int i = 0; i < m; ++i) p.cut_list[base + i] = cutbuf[wave][1 + i];
            cutbuf[wave][0] = 0;
        }
    };

    const long long n_items = p.frame_list ? (long long)*p.frame_count : p.n_frames;
    // The per-frame scalars (live symbols, offset, CFO) of the NEXT frame of this wavefront are fetched while the current frame is
    // received: read where they are used -- symbol count, branch, offset, CFO, one after the other -- they cost three to four
    // dependent round trips to HBM per frame before the first sample is even requested.
    const long long istep = (long long)gridDim.x * 4;
    // (A VGPR zero the compiler cannot fold keeps these wave-uniform loads per-lane loads: as scalar values they would be moved to
    // SGPRs, and waited for, right where they are issued.)
    const int vzero = pinned(0);
    long long f_n = 0; int ns_v = 0, off_v = 0; double fd_v = 0.0;
    auto fetch_scalars = [&](long long item) {
        if (item < n_items) {
            f_n = p.frame_list ? (long long)p.frame_list[item] : item;
            const long long fi = f_n + vzero;
            ns_v = p.nsym[fi];
            off_v = p.offset ? p.offset[fi] : 0;
            fd_v = p.f_delta ? p.f_delta[fi] : 0.0;
        }
    };
    fetch_scalars((long long)blockIdx.x * 4 + wave);
    for (long long item = (long long)blockIdx.x * 4 + wave; item < n_items; item += istep) {
        const long long f = f_n;
        const int ns = __builtin_amdgcn_readfirstlane(ns_v);
        const long long off = __builtin_amdgcn_readfirstlane(off_v);
        const double turns = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(fd_v)), __builtin_amdgcn_readfirstlane(__double2loint(fd_v))) * 0.15915494309189533577;
        fetch_scalars(item + istep);   // in flight until the next iteration reads them
        if (ns <= 0) { if (p.final_out && lane == 0) p.final_len[f] = 0; continue; } // wave-uniform
        const cf st = cfo_phasor(turns, 8);
        int keep = 0; // fused finish: bytes of this frame's output (known once the first group is demodulated)
        const cf *src = p.in + f * p.frame_stride + off;
        const long long avail = p.frame_len - off; // samples of the trimmed frame

        auto frame_body = [&](auto cut_tag) {
        constexpr bool CUT = decltype(cut_tag)::value;
        // estimate_channel (receiver.rs:212-229) on the 5 training blocks (chunks 5..9): H = mean_b FFT(block_b) / training
        // = FFT(mean_b block_b) / training.  Lane n sums sample n of the 5 derotated blocks, the wavefront transforms the 64
        // sums with one point per lane (lane_fft64), lane l then holds bin bitrev6(l): ONE transform per frame instead of a
        // whole 8-symbol group iteration.  1/H goes through the wave's LDS slab into the (t + 8 m) register layout.
        // The frame's round trips to HBM overlap instead of following one another: the first data group's samples are requested
        // right behind the training blocks (before the channel estimate is computed), every further group while the one before it
        // is transformed.
        // Every load is issued unconditionally, in straight-line code, from an address that is always mapped: loads under
        // exec-mask branches (or on one side of a branch that joins before their first use) make the compiler wait for
        // vmcnt(0) where the FIRST of them is used, i.e. for the prefetch as well.  Lanes of symbols past the frame's count
        // transform the frame's first samples: their image words are never stored.  CUT (a capture that ends inside the frame,
        // wave-uniform per frame) is a second instance of the whole body: there elements at or beyond frame_len read the frame's
        // first samples too and are zeroed where the registers are taken (zmask, bit m).
        const cf *safe = p.in + f * p.frame_stride + t;
        auto issue_group = [&](int k0, cf *v, unsigned &zmask) {
            const int count = ns - k0 < 8 ? ns - k0 : 8;
            const int n0 = (10 + k0 + s) * S + CP + t; // sample id of this lane's first point
            const cf *base = s < count ? src + n0 : safe;
            zmask = 0u;
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                const bool pad = CUT && s < count && (n0 + 8 * m) >= avail;
                v[m] = ld_cf(pad ? safe : base + 8 * m);
                if (CUT) zmask |= pad ? 1u << m : 0u;
            }
        };
        cf *ginv = ginv_all + wave * 64;
        cf v[8];
        unsigned zm = 0u;
        {
            cf tws[6]; // twiddles of the one-point-per-lane transform
            const int lq = pinned(lane); // per frame: keeps the six LDS addresses out of the loop-invariant registers (they spilled)
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                const int h = 32 >> q;
                const cf x = twl[(lq & (h - 1)) << q];
                tws[q] = (lane & h) ? x : make_float2(1.f, 0.f);
            }
            const int bin = bitrev6(lane);
            const cf invt = p.inv_training[bin]; // requested with the training blocks (read after the transform it is one more dependent round trip)
            const int nb = 5 * S + CP + lane;
            cf xb[5];
#pragma unroll
            for (int b = 0; b < 5; ++b) xb[b] = ld_cf((!CUT || (nb + S * b) < avail) ? src + nb + S * b : safe);
            issue_group(0, v, zm);
#pragma unroll
            for (int b = 0; b < 5; ++b) if (CUT && (nb + S * b) >= avail) xb[b] = make_float2(0.f, 0.f);
            cf acc;
            if (p.f_delta) { // sum_b x_b e^{-j phi (nb + 80 b)}: Horner in the 80-sample step, then this lane's phasor
                const cf s80 = cfo_phasor(turns, S), q0 = cfo_phasor(turns, nb);
                acc = cadd(cmul(xb[4], s80), xb[3]);
                acc = cadd(cmul(acc, s80), xb[2]);
                acc = cadd(cmul(acc, s80), xb[1]);
                acc = cadd(cmul(acc, s80), xb[0]);
                acc = cmul(acc, q0);
            } else acc = cadd(cadd(cadd(xb[4], xb[3]), cadd(xb[2], xb[1])), xb[0]);
            acc = lane_fft64(acc, lane, tws);
            cf h = cmul(acc, invt);
            h = make_float2(h.x * 0.2f, h.y * 0.2f);
            if (p.hk) p.hk[f * 64 + bin] = h;
            const float rn = __builtin_amdgcn_rcpf(h.x * h.x + h.y * h.y);
            wave_fence();    // the previous frame's last reads of this table are done
            ginv[bin] = make_float2(h.x * rn, -h.y * rn);            // 1 / H
            wave_fence();
        }
        for (int k0 = 0; k0 < ns; k0 += 8) { // data symbols, 8 at a time (chunks 10..)
            const int count = ns - k0 < 8 ? ns - k0 : 8;
            const int n0 = (10 + k0 + s) * S + CP + t; // sample id of this lane's first point
            cf vn[8];
            unsigned zn = 0u;
            issue_group(k0 + 8 < ns ? k0 + 8 : k0, vn, zn); // the next group (past the last one: this group again, never used)
            if (CUT && zm) {
#pragma unroll
                for (int m = 0; m < 8; ++m) if ((zm >> m) & 1u) v[m] = make_float2(0.f, 0.f);
            }
            if (p.f_delta) { // CFO derotation, sample ids count from the trimmed start (receiver.rs:44-50)
                cf ph = cfo_phasor(turns, n0);
#pragma unroll
                for (int m = 0; m < 8; ++m) { v[m] = cmul(v[m], ph); ph = cmul(ph, st); }
            }
            bfly8<false>(v);
#pragma unroll
            for (int r = 0; r < 8; ++r) buf[wr ^ r] = v[r];
#pragma unroll
            for (int m = 0; m < 8; ++m) v[m] = buf[8 * m + (t ^ m)];
#pragma unroll
            for (int r = 1; r < 8; ++r) v[r] = cmul(v[r], twl[r * t]);
            bfly8<false>(v);
#pragma unroll
            for (int m = 0; m < 8; ++m) v[m] = cmul(v[m], ginv[t + 8 * m]); // equalise (receiver.rs:68-70)
            cf rot = make_float2(1.f, 0.f);
            if (GUARD) {
                cf pv = make_float2(1.f, 0.f);
                pv = (t == 6) ? v[0] : pv;
                pv = (t == 1) ? v[3] : pv;
                pv = (t == 7) ? v[4] : pv;
                pv = (t == 2) ? v[7] : pv;
                const float trn = sum8_lanes(__ocml_atan2pi_f32(pv.y, pv.x)) * 0.125f; // mean pilot angle in turns -> hardware sin / cos
                rot = make_float2(__builtin_amdgcn_cosf(trn), -__builtin_amdgcn_sinf(trn)); // applied inside the demapper
            }
            for (int i = lane; i < REGION_DW; i += 64) img[i] = 0u;
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                const int bo = bofftab[m * 64 + lane];
                if (bo >= 0) {
                    const unsigned idx = GUARD ? demap_point_rot(v[m], rot, BPS) : demap_point(v[m], BPS);
                    or_field<BPS>(img, bo, idx);
                }
            }
            // the next group's samples leave the prefetch registers BEFORE this group's bytes are stored: loads and stores share the
            // in-order VM counter, so a wait for the loads placed behind the stores would wait for the stores as well
#pragma unroll
            for (int m = 0; m < 8; ++m) v[m] = vn[m];
            zm = zn;
            const int ndw = (count * SYM_BYTES + 3) / 4;   // (6-byte symbols: an odd count ends in half a dword; its upper half is zero in the image and lies inside the row)
            if (p.final_out) {
                wave_fence(); // the image is complete
                if (k0 == 0) { // bincode fixint little-endian u128 length (src/packets/mod.rs:20-32), then Vec::truncate
                    const unsigned long long lo = (unsigned long long)img[0] | ((unsigned long long)img[1] << 32);
                    const unsigned long long hi = (unsigned long long)img[2] | ((unsigned long long)img[3] << 32);
                    const int body = ns * SYM_BYTES - 16;
                    keep = OFDM_HEADER_KEEP(int, lo, hi, body);
                    if (lane == 0) p.final_len[f] = keep;
                }
                unsigned char *fo = p.final_out + f * p.final_stride;
                for (int i = lane; i < ndw; i += 64) {
                    const int ob = k0 * SYM_BYTES + 4 * i - 16; // final byte index of this dword
                    if (ob < 0 || ob >= keep) continue;
                    if (ob + 4 <= keep) *reinterpret_cast<unsigned *>(fo + ob) = img[i];
                    else for (int j = 0; ob + j < keep; ++j) fo[ob + j] = (unsigned char)(img[i] >> (8 * j));
                }
            } else {
                unsigned *dst = reinterpret_cast<unsigned *>(p.out + f * p.out_stride + (long long)k0 * SYM_BYTES);
                for (int i = lane; i < ndw; i += 64) dst[i] = img[i];
            }
        }
        };
        const bool whole = (long long)(10 + ns) * S <= avail; // wave-uniform
        if (MODE == 0) {
            if (whole) frame_body(std::false_type{});
            else if (lane == 0) { // left to the MODE 1 launch
                const int m = cutbuf[wave][0];
                cutbuf[wave][1 + m] = (int32_t)f;
                cutbuf[wave][0] = m + 1;
                if (m + 1 == 16) cut_flush();
            }
        } else if (MODE == 1) {
            if (!whole) frame_body(std::true_type{});
        } else {
            if (whole) frame_body(std::false_type{}); else frame_body(std::true_type{});
        }
    }
    if (MODE == 0 && lane == 0) cut_flush();
}

// split = the caller gave a cut-list workspace and no frame list of its own: MODE 0 over every frame, then MODE 1 over the frames it left
template <int BPS, bool GUARD> static hipError_t launch_rxframe(RxFrame64Params p, dim3 grid, hipStream_t st, bool split) {
    if (!split) { hipLaunchKernelGGL((k_rxframe64<BPS, GUARD, 2>), grid, dim3(256), 0, st, p); return hipGetLastError(); }
    hipError_t e = hipMemsetAsync(p.cut_count, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_rxframe64<BPS, GUARD, 0>), grid, dim3(256), 0, st, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    p.frame_list = p.cut_list; p.frame_count = p.cut_count;
    hipLaunchKernelGGL((k_rxframe64<BPS, GUARD, 1>), grid, dim3(256), 0, st, p); // the same persistent grid: a batch of captures that are ALL cut short must not crawl through 64 workgroups (an empty list costs microseconds either way)
    return hipGetLastError();
}

// Fused channel estimate + demod for N = 64 frames.  hipErrorNotSupported => caller uses run_chest + run_demod.
hipError_t run_rxframe64(const SymParams &sp, float2 *hk_out, hipStream_t st, int num_cu, unsigned char *final_out,
                         long long final_stride, int32_t *final_len, const int32_t *frame_list, const int32_t *frame_count,
                         int32_t *cut_ws) {
    const int nd = sp.guard ? 48 : 64;
    if ((nd * sp.bps) % 16 != 0 || !sp.nsym_frame || sp.soft) return hipErrorNotSupported;   // whole bytes per symbol, whole dwords per 8 symbols
    // raw rows are written with dword stores (the fused finish does not touch them)
    const bool to_final = final_out && final_len && (reinterpret_cast<uintptr_t>(final_out) & 3) == 0 && (final_stride & 3) == 0;
    if (!to_final && ((reinterpret_cast<uintptr_t>(sp.out_bytes) & 3) || (sp.out_stride & 3))) return hipErrorNotSupported;
    if (sp.n_frames <= 0) return hipSuccess;
    RxFrame64Params p;
    p.in = sp.in; p.n_frames = sp.n_frames; p.frame_stride = sp.frame_stride; p.frame_len = sp.frame_len;
    p.offset = sp.offset; p.f_delta = sp.f_delta; p.nsym = sp.nsym_frame; p.tw = sp.tw; p.inv_training = sp.inv_training;
    p.out = sp.out_bytes; p.out_stride = sp.out_stride; p.hk = hk_out;
    p.final_out = nullptr; p.final_stride = 0; p.final_len = nullptr;
    if (to_final) { p.final_out = final_out; p.final_stride = final_stride; p.final_len = final_len; }
    else if (final_out) return hipErrorNotSupported;
    p.frame_list = frame_list; p.frame_count = frame_count;
    // The split pays when cut captures are the exception (measured on 1 M config-3 frames, same box: chain 4.98 -> 4.68 ms / 4.98 -> 4.88 ms on
    // two boxes; with EVERY capture cut short the pair costs 18 % more than the one kernel: a skip pass plus the list): it is used when the
    // capture has room for the longest frame the caller asks for plus a 64-sample start offset -- what a slotted capture looks like.
    const bool roomy = sp.frame_len >= (long long)(10 + sp.syms_per_frame) * 80 + 64;
    const bool split = cut_ws != nullptr && frame_list == nullptr && roomy && !tuning_or_default(sp.tune).no_rxframe64_split;
    p.cut_count = split ? cut_ws : nullptr; p.cut_list = split ? cut_ws + 4 : nullptr;
    const dim3 grid((unsigned)persistent_grid((sp.n_frames + 3) / 4, frame_list ? 64 : (long long)num_cu * 8, tuning_or_default(sp.tune)));
    trace_add(sp.trace, frame_list ? "k_rxframe64<list>" : (p.final_out ? "k_rxframe64<finish>" : "k_rxframe64"));
    if (split) trace_add(sp.trace, "k_rxframe64<cut,list>");
    return with_bps(sp.bps, [&](auto B) { return with_bool(sp.guard != 0, [&](auto G) {
        return launch_rxframe<decltype(B)::value, decltype(G)::value>(p, grid, st, split); }); });
}

// ---------------------------------------------------------------------------------------------------------------
// k_txframe64: encode (src/transmitter.rs:11-58) for N = 64, one 256-thread workgroup per frame, ONE pass over HBM.
//   The data symbols are built in LDS (D x 80 samples): per group of 8 symbols a wavefront maps the byte stream to
//   constellation points straight into the Stockham input pattern (modulate + encode_block, transmitter.rs:108-165),
//   runs the inverse FFT64 in the k_demod64 layout (the symbol's own LDS slot doubles as the transpose slab), adds the
//   cyclic prefix (prefix_block, transmitter.rs:168-181) and tracks max(re, im).  After one barrier the workgroup knows
//   the frame's signed maximum (normalize, transmitter.rs:183-194, the constant header's maximum comes from the host)
//   and streams [header | data] / max to HBM with 16-byte stores.  HBM traffic: payload in, frame out, nothing else
//   (the two-kernel path wrote the frame, read it back and wrote it again).
struct TxFrame64Params {
    const uint8_t *payload;
    long long payload_stride;
    const int32_t *payload_len;
    int payload_bytes;
    long long n_frames;
    int n_sym;                 // data symbols per frame
    const float2 *tw;          // exp(-2 pi i m / 64)
    const float2 *header;      // 10 constant blocks (800 samples), unnormalised
    float header_max;
    float2 *out;
    long long out_stride;      // samples
    int debug;                 // OFDM_TX_DEBUG=1: the first two samples of every frame carry section times (s_memtime ticks)
};

template <int BPS, bool GUARD>
__global__ __launch_bounds__(256, 4) void k_txframe64(TxFrame64Params p) {
    constexpr int S = 80, CP = 16, HDR = 10 * S;
    constexpr int ND = GUARD ? 48 : 64;
    constexpr int SYM_BITS = ND * BPS;
    extern __shared__ __align__(16) unsigned char smem[];
    cf *hd = reinterpret_cast<cf *>(smem);                      // [800] the constant header, staged once
    cf *fb = hd + HDR;                                          // [ceil8(n_sym) * 80] data symbols, unnormalised
    const int groups = (p.n_sym + 7) >> 3;
    unsigned *mxw = reinterpret_cast<unsigned *>(fb + (size_t)groups * 8 * S); // [2] frame maximum (float bits, >= 0), by frame parity
    unsigned *sbw_all = mxw + 4;                                               // [2][groups * 128 + 8] the frame's byte stream as dwords, by frame parity
    const int sbw_dw = groups * 128 + 8;
    const int stream_dw = groups * 8 * (SYM_BITS / 8) / 4 + 1;  // dwords the mapper may touch (one dword of slack)

    const int tid = threadIdx.x, lane = tid & 63, nthr = blockDim.x, nwaves = nthr >> 6;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int s = lane >> 3, t = lane & 7;
    cf w[7];
#pragma unroll
    for (int r = 1; r < 8; ++r) { const cf x = p.tw[r * t]; w[r - 1] = make_float2(x.x, -x.y); } // conjugate: inverse transform
    int qoff[8]; // bit offset of bin (t + 8m)'s field inside one symbol's stream, -1 = null, -2 = pilot
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int c = t + 8 * m, cls = carrier_class64(c, GUARD);
        qoff[m] = cls == 0 ? (GUARD ? data_classes_below64(c) : c) * BPS : (cls == 2 ? -2 : -1);
    }
    const int wr = swz(8 * t);
    for (int i = tid; i < HDR; i += nthr) hd[i] = p.header[i];
    __shared__ float lvl[16]; // constellation levels by raw bit field, from axis_level itself (bit-identical): 2 LDS reads per point
    if (tid < 16) lvl[tid] = BPS > 1 && tid < (1 << (BPS >> 1)) ? axis_level((unsigned)tid, BPS >> 1) : 0.f;

    // The byte stream = 16-byte little-endian length (src/packets/mod.rs:20-32) + payload + zeros.  Dword i of the
    // PAYLOAD is fetched by thread (i mod nthr); the first two per thread are prefetched one frame ahead.
    const bool aligned = ((reinterpret_cast<uintptr_t>(p.payload) | (uintptr_t)p.payload_stride) & 3) == 0;
    auto pay_dword = [&](const uint8_t *pay, long long len, int i) -> unsigned { // payload bytes 4i .. 4i+3, zero past len
        const long long b0 = 4LL * i;
        if (b0 + 4 <= len && aligned) return reinterpret_cast<const unsigned *>(pay)[i];
        unsigned v = 0;
        for (int j = 0; j < 4; ++j) if (b0 + j < len) v |= (unsigned)pay[b0 + j] << (8 * j);
        return v;
    };
    // The prefetch is issued without a branch and without knowing the frame's length (a load under a branch, or behind the
    // scalar load of payload_len[f], is a synchronous one): dwords wholly inside the payload ROW (payload_bytes, mapped
    // whatever the frame's own length) are loaded as they are and cut to the frame's length when they are taken out of
    // the registers; the ragged last dword of a row whose size is not a multiple of 4 is rebuilt byte by byte there.
    // payload_len[f] itself travels with them as a per-lane load (a VGPR zero the compiler cannot fold keeps it off the
    // scalar unit, whose loads are waited for at the next LDS wait).
    const int vzero = pinned(0);
    const bool row0 = aligned && 4LL * tid + 4 <= p.payload_bytes, row1 = aligned && 4LL * (tid + nthr) + 4 <= p.payload_bytes;
    auto issue = [&](long long fr, unsigned &d0, unsigned &d1, int &ln) {
        const long long fc = fr < p.n_frames ? fr : p.n_frames - 1; // past the batch: any mapped row, the values are never used
        const uint8_t *row = p.payload + fc * p.payload_stride;
        d0 = *reinterpret_cast<const unsigned *>(row0 ? row + 4 * tid : reinterpret_cast<const uint8_t *>(p.tw));
        d1 = *reinterpret_cast<const unsigned *>(row1 ? row + 4 * (tid + nthr) : reinterpret_cast<const uint8_t *>(p.tw));
        ln = p.payload_len ? p.payload_len[fc + vzero] : p.payload_bytes;
    };
    auto settle = [&](unsigned raw, bool whole, const uint8_t *pay, long long len, int i) -> unsigned {
        const long long keep = len - 4LL * i;                    // payload bytes from this dword on
        if (whole) return keep >= 4 ? raw : (keep <= 0 ? 0u : raw & ((1u << (8 * (int)keep)) - 1u));
        return pay_dword(pay, len, i);
    };
    // Per frame: [barrier] map + IFFT out of this frame's byte stream -> next frame's bytes out of the prefetch registers
    // into the OTHER stream buffer, the frame after next's loads issued -> [barrier] normalise + store.  The prefetched
    // loads are waited for BEFORE this frame's stores are issued: loads and stores share the in-order VM counter, and a
    // wait placed after the stores (the round-2 layout took the registers at the top of the next frame) drains them all.
    auto fill = [&](unsigned *sbw, long long fr, unsigned d0, unsigned d1, long long len) {
        const uint8_t *pay = p.payload + fr * p.payload_stride;
        if (tid < 4) sbw[tid] = tid < 2 ? (unsigned)((unsigned long long)len >> (32 * tid)) : 0u;
        if (tid + 4 < stream_dw) sbw[4 + tid] = settle(d0, row0, pay, len, tid);
        if (tid + nthr + 4 < stream_dw) sbw[4 + tid + nthr] = settle(d1, row1, pay, len, tid + nthr);
        for (int i = tid + 2 * nthr; i + 4 < stream_dw; i += nthr) sbw[4 + i] = pay_dword(pay, len, i); // long payloads
    };
    long long f = blockIdx.x;
    unsigned pre0 = 0, pre1 = 0;
    int pre_len = 0;
    long long len = 0;
    int cur = 0;
    if (f < p.n_frames) {
        issue(f, pre0, pre1, pre_len);
        len = row_len(__builtin_amdgcn_readfirstlane(pre_len), p.payload_bytes);
        fill(sbw_all, f, pre0, pre1, len);
        issue(f + gridDim.x, pre0, pre1, pre_len);
    }
    if (tid < 2) mxw[tid] = 0u;
    for (; f < p.n_frames; f += gridDim.x, cur ^= 1) {
        lds_barrier(); // this frame's byte stream is complete; the previous frame has left LDS (and the header is staged)
        const long long t0 = kProfile && p.debug ? (long long)__builtin_amdgcn_s_memtime() : 0;
        const unsigned char *sb = reinterpret_cast<const unsigned char *>(sbw_all + cur * sbw_dw);
        long long t1 = 0;
        const int npoints = (int)(((16 + len) * 8 + BPS - 1) / BPS); // points that carry stream bits; the rest are 0
        float lmax = 0.f;
        for (int g = wave; g < groups; g += nwaves) {
            const int k = 8 * g + s;       // this lane's symbol
            cf *buf = fb + k * S;          // its LDS slot (80 >= 72 entries: also the transpose slab)
            cf v[8];
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                cf z = make_float2(0.f, 0.f);
                if (qoff[m] == -2) z = make_float2(1.f, 0.f);
                else if (qoff[m] >= 0) {
                    const int bit = k * SYM_BITS + qoff[m];
                    if (bit < npoints * BPS && k < p.n_sym) {
                        const unsigned two = (unsigned)sb[bit >> 3] | ((unsigned)sb[(bit >> 3) + 1] << 8);
                        const unsigned idx = (two >> (bit & 7)) & ((1u << BPS) - 1u);
                        z = BPS == 1 ? map_point(idx, 1) : make_float2(lvl[idx & ((1u << (BPS >> 1)) - 1u)], lvl[idx >> (BPS >> 1)]);
                    }
                }
                v[m] = z;
            }
            bfly8<true>(v);
#pragma unroll
            for (int r = 0; r < 8; ++r) buf[wr ^ r] = v[r];
#pragma unroll
            for (int m = 0; m < 8; ++m) v[m] = buf[8 * m + (t ^ m)];
#pragma unroll
            for (int r = 1; r < 8; ++r) v[r] = cmul(v[r], w[r - 1]);
            bfly8<true>(v);
            // v[q] = 64 x[t + 8q]; prefix_block: out = [x[48..64), x[0..64)]
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const cf y = make_float2(v[q].x * (1.0f / 64), v[q].y * (1.0f / 64));
                v[q] = y;
                lmax = fmaxf(lmax, fmaxf(y.x, y.y));
            }
            wave_fence(); // the slab reads above precede the overwrites below
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                buf[CP + t + 8 * q] = v[q];
                if (q >= 6) buf[t + 8 * q - 48] = v[q];
            }
        }
#pragma unroll
        for (int sh = 32; sh >= 1; sh >>= 1) lmax = fmaxf(lmax, __shfl_xor(lmax, sh, 64));
        if (lane == 0) atomicMax(&mxw[cur], __float_as_uint(lmax)); // non-negative floats order like their bit patterns
        if (kProfile && p.debug) t1 = (long long)__builtin_amdgcn_s_memtime();
        long long len_next = 0;
        if (f + gridDim.x < p.n_frames) { // workgroup-uniform
            len_next = row_len(__builtin_amdgcn_readfirstlane(pre_len), p.payload_bytes);
            fill(sbw_all + (cur ^ 1) * sbw_dw, f + gridDim.x, pre0, pre1, len_next);
        }
        if (tid == 0) mxw[cur ^ 1] = 0u; // last read in the previous frame's store phase, which every thread left before this frame's first barrier
        issue(f + 2LL * gridDim.x, pre0, pre1, pre_len);
        lds_barrier();
        const long long t2 = kProfile && p.debug ? (long long)__builtin_amdgcn_s_memtime() : 0;
        const float inv = 1.0f / fmaxf(p.header_max, __uint_as_float(mxw[cur])); // one divide per thread, then multiplies (<= 1 ulp)
        len = len_next;
        // stream [header | data] out: header and data are contiguous in LDS, two samples per 16-byte store
        const int total2 = (HDR + p.n_sym * S) >> 1;
        float4 *dst = reinterpret_cast<float4 *>(p.out + f * p.out_stride);
        const float4 *src4 = reinterpret_cast<const float4 *>(hd);
        int i = tid;
        for (; i + 3 * nthr < total2; i += 4 * nthr) {
            const float4 a = src4[i], b = src4[i + nthr], c = src4[i + 2 * nthr], d = src4[i + 3 * nthr];
            dst[i] = make_float4(a.x * inv, a.y * inv, a.z * inv, a.w * inv);
            dst[i + nthr] = make_float4(b.x * inv, b.y * inv, b.z * inv, b.w * inv);
            dst[i + 2 * nthr] = make_float4(c.x * inv, c.y * inv, c.z * inv, c.w * inv);
            dst[i + 3 * nthr] = make_float4(d.x * inv, d.y * inv, d.z * inv, d.w * inv);
        }
        for (; i < total2; i += nthr) { const float4 a = src4[i]; dst[i] = make_float4(a.x * inv, a.y * inv, a.z * inv, a.w * inv); }
        if (kProfile && p.debug) {
            __syncthreads();
            if (tid == 0) {
                const long long t3 = (long long)__builtin_amdgcn_s_memtime();
                dst[0] = make_float4((float)(t1 - t0), (float)(t2 - t1), (float)(t3 - t2), 0.f); // map + IFFT, next frame's bytes, stores
            }
        }
    }
}

template <int BPS, bool GUARD> static hipError_t launch_txframe(const TxFrame64Params &p, dim3 grid, size_t lds, hipStream_t st) {
    const int groups = (p.n_sym + 7) / 8;
    const dim3 block(64u * (unsigned)(groups < 4 ? groups : 4)); // one wavefront per 8-symbol group, at most four
    hipLaunchKernelGGL((k_txframe64<BPS, GUARD>), grid, block, lds, st, p);
    return hipGetLastError();
}
// Fused TX for N = 64 frames of up to 56 data symbols.  hipErrorNotSupported => caller uses k_sym<M_TX> + k_tx_finish.
hipError_t run_txframe64(const SymParams &sp, const float2 *header, float header_max, hipStream_t st, int num_cu) {
    const int n_sym = sp.syms_per_frame;
    if (n_sym <= 0 || n_sym > 56 || (!sp.payload && sp.payload_bytes)) return hipErrorNotSupported;
    if ((reinterpret_cast<uintptr_t>(sp.out) & 15) || (sp.out_stride_s & 1)) return hipErrorNotSupported; // 16-byte stores
    if (sp.n_frames <= 0) return hipSuccess;
    TxFrame64Params p;
    p.payload = sp.payload; p.payload_stride = sp.payload_stride; p.payload_len = sp.payload_len; p.payload_bytes = sp.payload_bytes;
    p.n_frames = sp.n_frames; p.n_sym = n_sym; p.tw = sp.tw; p.header = header; p.header_max = header_max;
    p.out = sp.out; p.out_stride = sp.out_stride_s;
    const Tuning &tu = tuning_or_default(sp.tune);
    p.debug = kProfile ? tu.debug_tx : 0;
    const int groups = (n_sym + 7) / 8;
    const size_t lds = (size_t)(800 + groups * 8 * 80) * sizeof(float2) + 16 + 2 * ((size_t)groups * 8 * 64 + 32); // header + frame + max + two byte streams
    long long per_cu = (long long)(160 * 1024) / (long long)lds;
    const int waves_per_cu = tu.tx_waves > 0 ? tu.tx_waves : 16; // tuning knob (measured best: 16)
    long long wave_cap = waves_per_cu / (groups < 4 ? groups : 4); // wavefronts per CU
    if (wave_cap < 1) wave_cap = 1;
    if (per_cu > wave_cap) per_cu = wave_cap;
    const dim3 grid((unsigned)persistent_grid(sp.n_frames, (long long)num_cu * per_cu, tu));
    trace_add(sp.trace, "k_txframe64");
    return with_bps(sp.bps, [&](auto B) { return with_bool(sp.guard != 0, [&](auto G) {
        return launch_txframe<decltype(B)::value, decltype(G)::value>(p, grid, lds, st); }); });
}

template <int BPS, bool GUARD, bool HK> static hipError_t launch_demod64(Fast64Params p, hipStream_t st, int num_cu, const Tuning &tu, Trace *trace) {
    p.debug = kProfile ? tu.debug_demod64 : 0;
    constexpr int region_bytes = (GUARD ? 48 : 64) * BPS;
    {   // 16-byte stores need 16-byte aligned group regions: base, frame stride and the 8-symbol region itself
        p.store_policy = tu.demod64_store_policy;
        p.wide_stores = !tu.demod64_narrow_stores && region_bytes % 16 == 0 && (reinterpret_cast<uintptr_t>(p.out) & 15) == 0 && (p.out_stride & 15) == 0;
    }
    // burst mode (config-2 shape only: the template is instantiated once): 4 groups per step, whole-line stores
    const bool burst = BPS == 6 && GUARD && !HK && tu.demod64_burst >= 4 && p.wide_stores && p.n_groups % 4 == 0 &&
                       p.out_stride == (long long)p.groups_per_frame * region_bytes && (reinterpret_cast<uintptr_t>(p.out) & 127) == 0;
    // 16 groups per burst where the batch divides (4.6 KB of stores per wavefront step; 37 KB of LDS per workgroup still leaves four
    // resident): 1.784 -> 1.761 ms per 1 M frames against bursts of 4 on a box of the slow population; Tuning::demod64_burst caps it (A/B)
    const int burst_cap = tu.demod64_burst;
    const int bl = !burst ? 1 : (burst_cap >= 16 && p.n_groups % 16 == 0) ? 16 : (burst_cap >= 8 && p.n_groups % 8 == 0) ? 8 : 4;
    auto kernel = !burst ? k_demod64<BPS, GUARD, HK, 1> : bl == 16 ? k_demod64<6, true, false, 16> : bl == 8 ? k_demod64<6, true, false, 8> : k_demod64<6, true, false, 4>;
    const long long units = burst ? p.n_groups / bl : p.n_groups;
    const int knob = tu.demod64_wg_per_cu; // tuning knob
    const int per_cu = knob > 0 ? knob : (resident_blocks(kernel, 256) >= 4 ? 8 : 2 * resident_blocks(kernel, 256));
    const int grid = (int)persistent_grid((units + 3) / 4, (long long)num_cu * per_cu, tu); // a workgroup = four waves, a unit each
    trace_add(trace, !burst ? "k_demod64" : bl == 16 ? "k_demod64<burst16>" : bl == 8 ? "k_demod64<burst8>" : "k_demod64<burst4>");
    p.stride_groups = (long long)grid * 4;
    const int gpf = p.groups_per_frame;
    p.f0 = 0; p.k0 = 0;
    p.blk_df = 4 / gpf; p.blk_dk = 4 % gpf;    // a block advances the group index by 4
    p.wave_df = 0; p.wave_dk = 1;              // a wave by 1 (normalised in the kernel)
    p.step_df = p.stride_groups / gpf; p.step_dk = (int)(p.stride_groups % gpf);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, st, p);
    return hipGetLastError();
}

// Returns hipErrorNotSupported when the request is outside the fast path's envelope (caller falls back to k_sym).
hipError_t run_demod64_fast(const SymParams &sp, hipStream_t st, int num_cu) {
    if (sp.offset || sp.f_delta || sp.nsym_frame || sp.soft) return hipErrorNotSupported;
    if (sp.syms_per_frame <= 0 || (sp.syms_per_frame & 7) != 0) return hipErrorNotSupported;
    if (sp.hk && sp.hk_stride != 0) return hipErrorNotSupported;
    if ((long long)(sp.first_symbol + sp.syms_per_frame) * 80 > sp.frame_len) return hipErrorNotSupported; // no tail padding
    if ((reinterpret_cast<uintptr_t>(sp.out_bytes) & 3) || (sp.out_stride & 3)) return hipErrorNotSupported;
    if (reinterpret_cast<uintptr_t>(sp.in) & 7) return hipErrorNotSupported;
    Fast64Params p;
    p.in = sp.in; p.frame_stride = sp.frame_stride; p.first_symbol = sp.first_symbol;
    p.hk = sp.hk; p.tw = sp.tw; p.out = sp.out_bytes; p.out_stride = sp.out_stride;
    p.groups_per_frame = sp.syms_per_frame / 8;
    p.n_groups = sp.n_frames * (long long)p.groups_per_frame;
    if (p.n_groups <= 0) return hipSuccess;
    const Tuning &tu = tuning_or_default(sp.tune);
    return with_bps(sp.bps, [&](auto B) { return with_bool(sp.guard != 0, [&](auto G) { return with_bool(p.hk != nullptr, [&](auto H) {
        return launch_demod64<decltype(B)::value, decltype(G)::value, decltype(H)::value>(p, st, num_cu, tu, sp.trace); }); }); });
}

} // namespace ofdm
