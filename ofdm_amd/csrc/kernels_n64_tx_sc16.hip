// kernels_n64_tx_sc16.hip -- EXT-10: k_txframe64_sc16, the N = 64 encode of kernels_n64.hip (k_txframe64) writing sc16 samples
// (interleaved little-endian int16 I/Q, 4 bytes a sample) for a DAC.
//
// k_txframe64's frame loop, unchanged: one workgroup owns a frame over a persistent grid; byte stream and data symbols are built in LDS
// (map, inverse FFT64 in the k_demod64 layout, cyclic prefix, signed maximum); the payload of the frame after next is prefetched and
// waited for before this frame's stores are issued; the LDS layout is k_txframe64's.  What differs is the store phase: [header | data]
// is contiguous in LDS and holds 80 (10 + D) samples, a whole number of groups of four.  A thread reads four samples (two 16-byte LDS
// reads), forms x * inv as k_txframe64 does, then sc16_mul(., scale) -- one rounded f32 product of its own (include/ofdm_hip.h, "sc16")
// -- rint, clamp and pack (sc16_narrow2, device_common.hpp), and issues ONE 16-byte store of four sc16 samples where k_txframe64 issues
// two 16-byte stores of two fc32 samples each: row f is ofdm_sc16_narrow(frame f of ofdm_tx_encode_batch, scale), bit for bit, in half
// the HBM bytes.
// Clipped components (normalize divides by the SIGNED maximum, so a frame's negative peak is not bounded by -1): every lane counts in a
// register, a wavefront adds its sum to one of two LDS words by frame parity -- the two spare words next to the frame maxima, mxw[2 + cur]
// -- and thread 0 stores the word of the PREVIOUS frame after this frame's second barrier, when every wavefront has left that frame's
// store phase, and clears it.  No barrier is added per frame; one more closes the last frame of a workgroup.  One plain store a frame,
// zero included; no global atomic, no memset in front of the launch.
// The body is a copy, not a shared __device__ function: k_txframe64's device code must stay what it is (tools/isa_identity.py), and its
// profiling exits (debug, kProfile) are not carried over.
// Roofline: HBM -- payload in, 4 bytes a sample out.
#include "device_common.hpp"
#include "kernels.hpp"
#include <type_traits>

namespace ofdm {

struct TxFrame64Sc16Params {
    const uint8_t *payload;
    long long payload_stride;
    const int32_t *payload_len;
    int payload_bytes;
    long long n_frames;
    int n_sym;                 // data symbols per frame
    const float2 *tw;          // exp(-2 pi i m / 64)
    const float2 *header;      // 10 constant blocks (800 samples), unnormalised
    float header_max;
    float scale;
    uint32_t *out;             // one dword = (int16 re, int16 im)
    long long out_stride;      // samples, a multiple of 4
    int32_t *clipped;          // optional: clipped components per frame
};

template <int BPS, bool GUARD>
__global__ __launch_bounds__(256, 4) void k_txframe64_sc16(TxFrame64Sc16Params p) {
    constexpr int S = 80, CP = 16, HDR = 10 * S;
    constexpr int ND = GUARD ? 48 : 64;
    constexpr int SYM_BITS = ND * BPS;
    extern __shared__ __align__(16) unsigned char smem[];
    cf *hd = reinterpret_cast<cf *>(smem);                      // [800] the constant header, staged once
    cf *fb = hd + HDR;                                          // [ceil8(n_sym) * 80] data symbols, unnormalised
    const int groups = (p.n_sym + 7) >> 3;
    unsigned *mxw = reinterpret_cast<unsigned *>(fb + (size_t)groups * 8 * S); // [2] frame maximum (float bits, >= 0), by frame parity
    unsigned *clw = mxw + 2;                                                   // [2] clipped components, by frame parity
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

    // The byte stream, its prefetch and its settling are k_txframe64's (kernels_n64.hip explains the branch-free prefetch).
    const bool aligned = ((reinterpret_cast<uintptr_t>(p.payload) | (uintptr_t)p.payload_stride) & 3) == 0;
    auto pay_dword = [&](const uint8_t *pay, long long len, int i) -> unsigned { // payload bytes 4i .. 4i+3, zero past len
        const long long b0 = 4LL * i;
        if (b0 + 4 <= len && aligned) return reinterpret_cast<const unsigned *>(pay)[i];
        unsigned v = 0;
        for (int j = 0; j < 4; ++j) if (b0 + j < len) v |= (unsigned)pay[b0 + j] << (8 * j);
        return v;
    };
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
    if (tid < 4) mxw[tid] = 0u; // both maxima and both clipped counts
    const long long f_first = f;
    for (; f < p.n_frames; f += gridDim.x, cur ^= 1) {
        lds_barrier(); // this frame's byte stream is complete; the previous frame has left LDS (and the header is staged)
        const unsigned char *sb = reinterpret_cast<const unsigned char *>(sbw_all + cur * sbw_dw);
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
        long long len_next = 0;
        if (f + gridDim.x < p.n_frames) { // workgroup-uniform
            len_next = row_len(__builtin_amdgcn_readfirstlane(pre_len), p.payload_bytes);
            fill(sbw_all + (cur ^ 1) * sbw_dw, f + gridDim.x, pre0, pre1, len_next);
        }
        if (tid == 0) mxw[cur ^ 1] = 0u; // last read in the previous frame's store phase, which every thread left before this frame's first barrier
        issue(f + 2LL * gridDim.x, pre0, pre1, pre_len);
        lds_barrier();
        const float inv = 1.0f / fmaxf(p.header_max, __uint_as_float(mxw[cur])); // one divide per thread, then multiplies (<= 1 ulp)
        len = len_next;
        // the previous frame's clipped count: every wavefront added to clw[cur ^ 1] before it reached this frame's first barrier, and
        // nothing adds to it again before the next frame's second one
        if (tid == 0 && f != f_first) {
            if (p.clipped) p.clipped[f - gridDim.x] = (int32_t)clw[cur ^ 1];
            clw[cur ^ 1] = 0u;
        }
        // stream [header | data] out: header and data are contiguous in LDS, four samples per 16-byte store
        const int total4 = (HDR + p.n_sym * S) >> 2;
        uint4 *dst = reinterpret_cast<uint4 *>(p.out + f * p.out_stride);
        const float4 *src4 = reinterpret_cast<const float4 *>(hd);
        int clipped = 0;
        auto pack4 = [&](const float4 a, const float4 b) -> uint4 { // x * inv exactly as k_txframe64 forms it, then the narrow rule
            uint4 d;
            d.x = sc16_narrow2(make_float2(a.x * inv, a.y * inv), p.scale, &clipped);
            d.y = sc16_narrow2(make_float2(a.z * inv, a.w * inv), p.scale, &clipped);
            d.z = sc16_narrow2(make_float2(b.x * inv, b.y * inv), p.scale, &clipped);
            d.w = sc16_narrow2(make_float2(b.z * inv, b.w * inv), p.scale, &clipped);
            return d;
        };
        int i = tid;
        for (; i + nthr < total4; i += 2 * nthr) {
            const float4 a0 = src4[2 * i], a1 = src4[2 * i + 1], b0 = src4[2 * (i + nthr)], b1 = src4[2 * (i + nthr) + 1];
            dst[i] = pack4(a0, a1);
            dst[i + nthr] = pack4(b0, b1);
        }
        for (; i < total4; i += nthr) dst[i] = pack4(src4[2 * i], src4[2 * i + 1]);
        if (p.clipped) { // an integer count: any order of the additions gives the same number
#pragma unroll
            for (int sh = 32; sh >= 1; sh >>= 1) clipped += __shfl_xor(clipped, sh, 64);
            if (lane == 0 && clipped) atomicAdd(&clw[cur], (unsigned)clipped);
        }
    }
    if (p.clipped && f_first < p.n_frames) { // the workgroup's last frame (cur was flipped once more on the way out)
        lds_barrier();
        if (tid == 0) p.clipped[f - gridDim.x] = (int32_t)clw[cur ^ 1];
    }
}

template <int BPS, bool GUARD> static hipError_t launch_txframe_sc16(const TxFrame64Sc16Params &p, dim3 grid, size_t lds, hipStream_t st) {
    const int groups = (p.n_sym + 7) / 8;
    const dim3 block(64u * (unsigned)(groups < 4 ? groups : 4)); // one wavefront per 8-symbol group, at most four
    hipLaunchKernelGGL((k_txframe64_sc16<BPS, GUARD>), grid, block, lds, st, p);
    return hipGetLastError();
}
// The envelope, stated once: run_txframe64's frames (1 .. 56 data symbols) with a 16-byte aligned sc16 output whose rows are a multiple
// of 4 samples apart (16-byte stores of four samples).  The caller asks BEFORE it runs the coding layers, so that a call outside it
// codes its rows once, on the two-pass path.
bool txframe64_sc16_takes(int n_sym, const void *out16, long long out_stride) {
    return n_sym >= 1 && n_sym <= 56 && (reinterpret_cast<uintptr_t>(out16) & 15) == 0 && (out_stride & 3) == 0;
}
// run_txframe64's grid (kernels_n64.hip)
hipError_t run_txframe64_sc16(const SymParams &sp, const float2 *header, float header_max, uint32_t *out16, long long out_stride, float scale,
                              int32_t *clipped, hipStream_t st, int num_cu) {
    const int n_sym = sp.syms_per_frame;
    if (!txframe64_sc16_takes(n_sym, out16, out_stride) || (!sp.payload && sp.payload_bytes)) return hipErrorNotSupported;
    if (sp.n_frames <= 0) return hipSuccess;
    TxFrame64Sc16Params p;
    p.payload = sp.payload; p.payload_stride = sp.payload_stride; p.payload_len = sp.payload_len; p.payload_bytes = sp.payload_bytes;
    p.n_frames = sp.n_frames; p.n_sym = n_sym; p.tw = sp.tw; p.header = header; p.header_max = header_max;
    p.scale = scale; p.out = out16; p.out_stride = out_stride; p.clipped = clipped;
    const Tuning &tu = tuning_or_default(sp.tune);
    const int groups = (n_sym + 7) / 8;
    const size_t lds = (size_t)(800 + groups * 8 * 80) * sizeof(float2) + 16 + 2 * ((size_t)groups * 8 * 64 + 32); // header + frame + max / clipped + two byte streams
    long long per_cu = (long long)(160 * 1024) / (long long)lds;
    const int waves_per_cu = tu.tx_waves > 0 ? tu.tx_waves : 16;
    long long wave_cap = waves_per_cu / (groups < 4 ? groups : 4); // wavefronts per CU
    if (wave_cap < 1) wave_cap = 1;
    if (per_cu > wave_cap) per_cu = wave_cap;
    const dim3 grid((unsigned)persistent_grid(sp.n_frames, (long long)num_cu * per_cu, tu));
    trace_add(sp.trace, "k_txframe64_sc16");
    return with_bps(sp.bps, [&](auto B) { return with_bool(sp.guard != 0, [&](auto G) {
        return launch_txframe_sc16<decltype(B)::value, decltype(G)::value>(p, grid, lds, st); }); });
}

} // namespace ofdm
