// kernels_conv.hip -- the constraint-length-7, rate-1/2 convolutional code (generators 133 / 171 octal, the 802.11a / DVB-T / DAB
// code; OFDM_ECC_CONV_K7, include/ofdm_hip.h, DESIGN.md section 3, EXT-2 convolutional code; restated in tests/conv_ref.py).
//   k_conv_encode   one thread per coded byte: four trellis steps, ten input bits out of two payload bytes.
//   k_viterbi_k7    one wavefront per frame, lane s = trellis state s.  Forward pass: int32 path metrics in one VGPR, the two
//                   predecessor metrics by ds_bpermute, one survivor decision per lane and step, shifted into a dword that leaves
//                   every 32 steps with one coalesced store into the wavefront's own survivor slab (workspace, sized by the
//                   grid).  Traceback: one coalesced load per 32 steps, the wave-uniform state walked with v_readlane and
//                   scalar bit tests.  Everything is exact integer arithmetic.
//   k_conv_encode_p the punctured encoder (rates 1/2, 2/3, 3/4) and the framed stream [length block][body] of the
//                   OFDM_ECC_CONV_K7F_* modes: one thread per output byte, every output bit mapped back to (step, A or B).
//   k_viterbi_k7f   k_viterbi_k7 with a punctured LLR fetch (LLR 0 at a dropped position); in chain mode the wavefront decodes the
//                   72-step length block, checks it, then decodes the body.  (Restated in tests/framed_ref.py.)
#include "device_common.hpp"
#include "kernels.hpp"

namespace ofdm {

constexpr unsigned kConvG0 = 0133, kConvG1 = 0171;

// outputs of the encoder register r = (u_t << 6) | state: A in bit 0, B in bit 1
__device__ __forceinline__ unsigned conv_outputs(unsigned r) {
    return (__popc(r & kConvG0) & 1u) | ((__popc(r & kConvG1) & 1u) << 1);
}

// coded byte j of a row covers steps 4j .. 4j + 3 = input bits 4j - 6 .. 4j + 3: payload bytes j / 2 - 1 and j / 2.  Bytes at or past
// the row's own length read 0 (the tail byte, and whatever follows it in the slot).
__global__ __launch_bounds__(256) void k_conv_encode(const uint8_t *in, long long n_frames, long long in_stride, const int32_t *in_len,
                                                     long long n_bytes, uint8_t *out, long long out_stride, int32_t *out_len) {
    const long long row = 2 * (n_bytes + 1), total = n_frames * row;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long f = i / row, j = i - f * row, b = j >> 1;
        const long long len = in_len ? row_len(in_len[f], (int)n_bytes) : n_bytes;
        const uint8_t *src = in + f * in_stride;
        const unsigned cur = b < len ? src[b] : 0u, prev = (b >= 1 && b - 1 < len) ? src[b - 1] : 0u;
        const unsigned w = (cur << 8) | prev;          // bit k = input bit 8 (b - 1) + k
        const int j0 = (int)(j & 1) * 4;
        unsigned byte = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) byte |= conv_outputs((w >> (j0 + k + 2)) & 0x7Fu) << (2 * k);
        out[f * out_stride + j] = (uint8_t)byte;
        if (out_len && j == 0) out_len[f] = (int32_t)(2 * (len + 1));
    }
}
hipError_t run_conv_encode(const uint8_t *in, long long n_frames, long long in_stride, const int32_t *in_len, long long n_bytes,
                           uint8_t *out, long long out_stride, int32_t *out_len, hipStream_t st) {
    if (n_frames <= 0) return hipSuccess;
    const long long total = n_frames * 2 * (n_bytes + 1);
    long long g = (total + 255) / 256;
    if (g > 2048LL * 8) g = 2048LL * 8;
    hipLaunchKernelGGL(k_conv_encode, dim3((unsigned)g), dim3(256), 0, st, in, n_frames, in_stride, in_len, n_bytes, out, out_stride,
                       out_len);
    return hipGetLastError();
}

// The punctured encoder and the framed stream.  Output byte j of a row: j < head is byte j of the length block, the unpunctured code
// of [u32 LE len][u32 LE ~len][0x00]; the others are the body.  Body bit q (LSB first) maps back to (step t, A or B) by the closed
// form of the keep mask: rate 1/2 q = 2 t + sel; rate 2/3 q = 3 g + m -> t = 2 g + (m == 2), B iff m == 1; rate 3/4 q = 4 g + m ->
// t = 3 g + (m < 2 ? 0 : m - 1), B iff m is odd.  Bits at or past the row's own conv_kept_bits(8 (len + 1)) are zero (the padding
// of the last byte, and whatever follows it in the slot).
__global__ __launch_bounds__(256) void k_conv_encode_p(const uint8_t *in, long long n_frames, long long in_stride, const int32_t *in_len,
                                                       long long n_bytes, int rate, int head, uint8_t *out, long long out_stride,
                                                       int32_t *out_len) {
    const long long row = head + conv_body_len(n_bytes, rate), total = n_frames * row;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long f = i / row, j = i - f * row;
        const long long len = in_len ? row_len(in_len[f], (int)n_bytes) : n_bytes;
        unsigned byte = 0;
        if (j < head) {
            const unsigned long long v = (unsigned long long)(unsigned)len | ((unsigned long long)~(unsigned)len << 32);
            const int lo = 4 * (int)j - 6;               // steps 4j .. 4j + 3 read input bits lo .. lo + 9
            const unsigned w = (unsigned)(lo < 0 ? v << -lo : v >> lo) & 0x3FFu;
#pragma unroll
            for (int k = 0; k < 4; ++k) byte |= conv_outputs((w >> k) & 0x7Fu) << (2 * k);
        } else {
            const long long q0 = 8 * (j - head), kept = conv_kept_bits(8 * (len + 1), rate);
            auto step_of = [&](long long q, unsigned &sel) -> long long {
                if (rate == 1) { const long long g = q / 3; const int m = (int)(q - 3 * g); sel = m == 1; return 2 * g + (m == 2); }
                if (rate == 2) { const long long g = q >> 2; const int m = (int)(q & 3); sel = m & 1; return 3 * g + (m < 2 ? 0 : m - 1); }
                sel = (unsigned)(q & 1); return q >> 1;
            };
            unsigned sel;
            const long long b0 = step_of(q0, sel) >> 3;    // the eight bits lie within steps 8 b0 .. 8 b0 + 13
            const uint8_t *src = in + f * in_stride;
            unsigned w = 0;                               // bit k = input bit 8 (b0 - 1) + k
#pragma unroll
            for (int k = 0; k < 4; ++k) { const long long b = b0 - 1 + k; if (b >= 0 && b < len) w |= (unsigned)src[b] << (8 * k); }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const long long t = step_of(q0 + k, sel);
                const unsigned r = (w >> (int)(t - 8 * b0 + 2)) & 0x7Fu;
                const unsigned bit = __popc(r & (sel ? kConvG1 : kConvG0)) & 1u;
                if (q0 + k < kept) byte |= bit << k;
            }
        }
        out[f * out_stride + j] = (uint8_t)byte;
        if (out_len && j == 0) out_len[f] = (int32_t)(head + conv_body_len(len, rate));
    }
}
hipError_t run_conv_encode_p(const uint8_t *in, long long n_frames, long long in_stride, const int32_t *in_len, long long n_bytes, int rate,
                             int head, uint8_t *out, long long out_stride, int32_t *out_len, hipStream_t st) {
    if (n_frames <= 0) return hipSuccess;
    const long long total = n_frames * (head + conv_body_len(n_bytes, rate));
    if (total <= 0) return hipSuccess;
    long long g = (total + 255) / 256;
    if (g > 2048LL * 8) g = 2048LL * 8;
    hipLaunchKernelGGL(k_conv_encode_p, dim3((unsigned)g), dim3(256), 0, st, in, n_frames, in_stride, in_len, n_bytes, rate, head, out,
                       out_stride, out_len);
    return hipGetLastError();
}

// One frame on one wavefront (all 64 lanes active).  llr: 2 T LLRs, positive = bit 1; the first n_out <= T / 8 decoded bytes go to
// out; surv: this wavefront's slab, 64 dwords per 32 steps.  T, terminated and n_out are wave-uniform.
//
// Branch metrics.  Lane = state s' at t + 1: input u = s' >> 5, predecessors p0 = (s' & 31) << 1 and p1 = p0 | 1.  Both generators
// tap delay 0 and delay 6, so the branch from p1 carries the complement of the outputs of the branch from p0: bm(p1) = -bm(p0),
// and bm(p0) is one of +-(La + Lb), +-(La - Lb).  The lane that fetched a step's LLR pair packs La + Lb and La - Lb into one
// dword; a step broadcasts it with one v_readlane, every lane takes its field (v_bfe_i32 at a per-lane offset) and applies its
// sign inside the two multiply-adds that form the candidates.
// Survivors.  Every lane shifts its own decision bit into a dword; after 32 steps the 64 dwords leave with one 256-byte store
// (8 bytes per step, as one 64-bit mask per step would take).  The traceback reads a block back with one load (lane = state) and
// picks the word of the wave-uniform state with v_readlane; the block below is in flight meanwhile.
//
// fetch(t, la, lb) loads the LLR pair of step t (the unpunctured one reads 2 t and 2 t + 1); sink(blk, bits) receives the decoded
// bits of steps 32 blk .. 32 blk + 31 (wave-uniform, bit j = u_{32 blk + j}), from the last block down to block 0.
struct FetchPair {
    const int8_t *llr;
    __device__ __forceinline__ void operator()(long long t, int &la, int &lb) const { la = llr[2 * t]; lb = llr[2 * t + 1]; }
};
struct SinkBytes {
    uint8_t *out; int n_out, lane;
    __device__ __forceinline__ void operator()(int blk, unsigned bits) const {
        const int b = blk * 4 + lane;
        if (lane < 4 && b < n_out) out[b] = (uint8_t)(bits >> (8 * lane));
    }
};
template <class Fetch, class Sink>
__device__ __forceinline__ void viterbi_k7_run(const Fetch &fetch, int T, bool terminated, Sink &sink, unsigned *surv, int lane) {
    const unsigned r0 = ((unsigned)(lane >> 5) << 6) | ((unsigned)(lane & 31) << 1);
    const int pa = __popc(r0 & kConvG0) & 1, pb = __popc(r0 & kConvG1) & 1;   // outputs (a, b) of the branch p0 -> s'
    const int sg = 2 * pa - 1, nsg = -sg;                 // bm(p0) = sg * (La + Lb) if a == b, sg * (La - Lb) otherwise
    const unsigned field = pa == pb ? 16u : 0u;
    const int a0 = (lane & 31) << 3, a1 = a0 | 4;         // ds_bpermute byte addresses of lanes p0, p1
    int pm = lane == 0 ? 0 : -(1 << 30);                  // every state but 0 is excluded at t = 0 (T <= 2^20 steps of at most 256 each)
    const long long last = T > 0 ? T - 1 : 0;
    long long tl = lane < last ? lane : last;             // (clamped: the load needs no branch, steps past T are never read)
    int la = 0, lb = 0;
    if (T > 0) fetch(tl, la, lb);
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int pq = (int)(((unsigned)(la + lb) << 16) | ((unsigned)(la - lb) & 0xFFFFu));
        tl = (long long)t0 + 64 + lane;                   // the next 64 steps' LLRs are in flight while these run
        tl = tl < last ? tl : last;
        fetch(tl, la, lb);
        const int pq_hi = __shfl_xor(pq, 32, 64);       // the second 32 steps, brought to lanes 0 .. 31
        for (int h = 0; h < 64 && t0 + h < T; h += 32) {
            const int n = __builtin_amdgcn_readfirstlane(T - t0 - h < 32 ? T - t0 - h : 32);
            const int pqh = h ? pq_hi : pq;
            unsigned dv = 0;
            auto step = [&](int i) __attribute__((always_inline)) {
                const int v = __builtin_amdgcn_sbfe(__builtin_amdgcn_readlane(pqh, i), field, 16u);
                const int c0 = __mul24(v, sg) + __builtin_amdgcn_ds_bpermute(a0, pm);
                const int c1 = __mul24(v, nsg) + __builtin_amdgcn_ds_bpermute(a1, pm);
                const bool d = c1 > c0;                   // a tie keeps p0
                pm = d ? c1 : c0;
                dv = (dv << 1) | (d ? 1u : 0u);           // step i of an n-step block: bit n - 1 - i
            };
            if (n == 32) {                                // a whole block: constant trip count, unrolled (the cross-lane operations
#pragma unroll                                            // rule out unrolling a loop of unknown length)
                for (int i = 0; i < 32; ++i) step(i);
            } else {
                for (int i = 0; i < n; ++i) step(i);
            }
            surv[(size_t)((t0 + h) >> 5) * 64 + lane] = dv;
        }
    }
    if (T <= 0) return;
    int s = 0;
    if (!terminated) {                                    // the largest final metric, lowest state on a tie
        int mx = pm;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { const int v = __shfl_xor(mx, o, 64); mx = v > mx ? v : mx; }
        s = __ffsll((long long)__ballot(pm == mx)) - 1;
    }
    // The state is the last six inputs (u_t = s_{t+1} >> 5), so stepping back shifts one decision in at the bottom: s_t =
    // ((s_{t+1} & 31) << 1) | decision, i.e. the decision of step t IS u_{t-6}.  Kept in one shift register `hist` (its low six bits
    // = the state), the walk leaves the decoded bits behind it in output order: after the block that starts at step t0, bit 6 + j
    // of hist is u_{t0 + j}.
    unsigned long long hist = (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane(s);
    int blk = (T - 1) >> 5;
    unsigned wv = surv[(size_t)blk * 64 + lane];
    for (; blk >= 0; --blk) {
        const int n = __builtin_amdgcn_readfirstlane(T - 32 * blk < 32 ? T - 32 * blk : 32);
        const int cur = (int)wv;
        if (blk > 0) wv = surv[(size_t)(blk - 1) * 64 + lane];
        auto back = [&](int pos) __attribute__((always_inline)) {   // step 32 blk + n - 1 - pos: bit pos of the state's decision word
            const unsigned word = (unsigned)__builtin_amdgcn_readlane(cur, (int)((unsigned)hist & 63u));
            hist = (hist << 1) | ((word >> pos) & 1u);
        };
        if (n == 32) {
#pragma unroll
            for (int pos = 0; pos < 32; ++pos) back(pos);
        } else {
            for (int pos = 0; pos < n; ++pos) back(pos);
        }
        sink(blk, (unsigned)(hist >> 6));
    }
}
__device__ __forceinline__ void viterbi_k7_frame(const int8_t *llr, int T, bool terminated, uint8_t *out, int n_out, unsigned *surv,
                                                 int lane) {
    const FetchPair fetch{llr};
    SinkBytes sink{out, n_out, lane};
    viterbi_k7_run(fetch, T, terminated, sink, surv, lane);
}

// Stage mode (raw == nullptr): every row decodes n_steps steps from its LLR 0, `terminated` as given, n_steps / 8 bytes out.
// Chain mode: the length header is read from the frame's hard bytes exactly as k_rx_finish reads it (keep = the header's value if it
// is below body, else body); T = 4 keep steps over LLRs 128 .. 128 + 8 keep, terminated iff the frame was not cut short, and
// out_len = max(keep / 2 - 1, 0): the tail byte is not delivered.
__global__ __launch_bounds__(256) void k_viterbi_k7(ViterbiParams p) {
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (long long)gridDim.x * 4;
    unsigned *surv = reinterpret_cast<unsigned *>(p.surv + wave * p.slab_words);
    for (long long f = wave; f < p.n_frames; f += n_waves) {
        const int8_t *l = p.llr + f * p.llr_stride;
        uint8_t *dst = p.out + f * p.out_stride;
        if (!p.raw) {
            viterbi_k7_frame(l, p.n_steps, p.terminated != 0, dst, p.n_steps >> 3, surv, lane);
            continue;
        }
        if (p.status[f] != 0) { if (lane == 0) p.out_len[f] = 0; continue; }
        const uint8_t *src = p.raw + f * p.raw_stride;
        const long long body = (long long)p.nsym[f] * p.bytes_per_symbol - 16;
        unsigned long long lo = 0, hi = 0;
        OFDM_HEADER_READ_BYTES(src, lo, hi) // (byte by byte whatever the row's alignment)
        long long keep = OFDM_HEADER_KEEP(long long, lo, hi, body);
        const bool whole = OFDM_HEADER_WHOLE(lo, hi, body);
        keep = __builtin_amdgcn_readfirstlane((int)keep);
        const int n_out = keep / 2 >= 1 ? (int)(keep / 2) - 1 : 0;
        viterbi_k7_frame(l + 128, (int)(4 * keep), __builtin_amdgcn_readfirstlane((int)whole) != 0, dst, n_out, surv, lane);
        if (lane == 0) p.out_len[f] = n_out;
    }
}

// Grid and slab for frames of at most max_steps steps: one survivor slab (8 bytes per step) per resident wavefront, the whole
// survivor workspace kept under 1 GiB by running fewer wavefronts when the frames are long.
void viterbi_k7_plan(long long n_frames, long long max_steps, int num_cu, const Tuning *tune, long long *blocks, long long *slab_words) {
    const long long words = ((max_steps > 0 ? max_steps : 1) + 63) & ~63LL;
    long long by_memory = (1LL << 30) / (words * 8 * 4);
    if (by_memory < 1) by_memory = 1;
    long long resident = 8LL * num_cu;               // 256 threads, 8 workgroups per CU: 8 wavefronts per SIMD
    if (resident > by_memory) resident = by_memory;
    *blocks = persistent_grid((n_frames + 3) / 4, resident, tuning_or_default(tune));
    if (*blocks < 1) *blocks = 1;
    *slab_words = words;
}
hipError_t run_viterbi_k7(const ViterbiParams &p, long long blocks, hipStream_t st) {
    if (p.n_frames <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_viterbi_k7, dim3((unsigned)blocks), dim3(256), 0, st, p);
    return hipGetLastError();
}

// The LLR pair of step t of a punctured row: rate 2/3, t = 2 g + r: A at 3 g + 2 r, B at 3 g + 1 iff r = 0; rate 3/4, t = 3 g + r:
// A at 4 g + (r ? 2 : 0) unless r = 2, B at 4 g + (r ? 3 : 1) unless r = 1.  A dropped position is LLR 0; its load re-reads the kept
// one, so nothing outside the row's conv_kept_bits(T) LLRs is touched.  (t < 2^20.)
struct FetchPunctured {
    const int8_t *llr; int rate;
    __device__ __forceinline__ void operator()(long long t, int &la, int &lb) const {
        const unsigned u = (unsigned)t;
        unsigned ia = 2 * u, ib = 2 * u + 1;
        bool ka = true, kb = true;
        if (rate == 1) {
            const unsigned g = u >> 1, r = u & 1;
            ia = 3 * g + 2 * r; kb = r == 0; ib = kb ? ia + 1 : ia;
        } else if (rate == 2) {
            const unsigned g = u / 3, r = u - 3 * g, base = 4 * g;
            ka = r != 2; kb = r != 1;
            ia = base + (r ? 2u : 0u); ib = base + (r ? 3u : 1u);
            if (!ka) ia = ib;
            if (!kb) ib = ia;
        }
        const int a = llr[ia], b = llr[ib];
        la = ka ? a : 0; lb = kb ? b : 0;
    }
};
// the 72 decoded bits of a length block
struct SinkLength {
    unsigned w0 = 0, w1 = 0, w2 = 0;
    __device__ __forceinline__ void operator()(int blk, unsigned bits) { if (blk == 0) w0 = bits; else if (blk == 1) w1 = bits; else w2 = bits; }
};

// Stage mode (status_rw == nullptr): every row decodes n_steps steps from its conv_kept_bits(n_steps, rate) LLRs.
// Chain mode (the framed modes): body = the demodulated bytes behind the legacy 16-byte header, which is not read.  body < 18 or an
// invalid length block (72 steps, terminated, LLRs 128 .. 272; valid iff bytes 4..7 complement bytes 0..3 and the tail byte is 0):
// status = OFDM_FRAME_HEADER, out_len = 0.  Otherwise the body is decoded from LLR 272 on: 8 (p + 1) steps, terminated, p bytes out
// if its conv_body_len(p) bytes are there, else the largest T' whose kept bits are there, unterminated, min(p, T' / 8) bytes out.
__global__ __launch_bounds__(256) void k_viterbi_k7f(ViterbiFParams p) {
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (long long)gridDim.x * 4;
    unsigned *surv = reinterpret_cast<unsigned *>(p.surv + wave * p.slab_words);
    for (long long f = wave; f < p.n_frames; f += n_waves) {
        const int8_t *l = p.llr + f * p.llr_stride;
        uint8_t *dst = p.out + f * p.out_stride;
        if (!p.status_rw) {
            const FetchPunctured fetch{l, p.rate};
            SinkBytes sink{dst, p.n_steps >> 3, lane};
            viterbi_k7_run(fetch, p.n_steps, p.terminated != 0, sink, surv, lane);
            continue;
        }
        if (p.status_rw[f] != 0) { if (lane == 0) p.out_len[f] = 0; continue; }
        const long long avail = (long long)p.nsym[f] * p.bytes_per_symbol - 16 - kConvLengthBlock;
        bool ok = avail >= 0;
        unsigned len = 0;
        if (ok) {
            const FetchPair fetch{l + 128};
            SinkLength head;
            viterbi_k7_run(fetch, 4 * kConvLengthBlock, true, head, surv, lane);
            ok = head.w1 == ~head.w0 && (head.w2 & 0xFFu) == 0;
            len = head.w0;
        }
        if (!ok) { if (lane == 0) { p.status_rw[f] = -4; p.out_len[f] = 0; } continue; }   // OFDM_FRAME_HEADER
        const bool whole = conv_body_len((long long)len, p.rate) <= avail;
        const long long steps = whole ? 8 * ((long long)len + 1) : conv_max_steps(8 * avail, p.rate);
        const long long bytes = whole || (long long)len < (steps >> 3) ? (long long)len : steps >> 3;
        const int T = __builtin_amdgcn_readfirstlane((int)steps), n_out = __builtin_amdgcn_readfirstlane((int)bytes);
        const FetchPunctured fetch{l + 128 + 8 * kConvLengthBlock, p.rate};
        SinkBytes sink{dst, n_out, lane};
        viterbi_k7_run(fetch, T, __builtin_amdgcn_readfirstlane((int)whole) != 0, sink, surv, lane);
        if (lane == 0) p.out_len[f] = n_out;
    }
}
hipError_t run_viterbi_k7f(const ViterbiFParams &p, long long blocks, hipStream_t st) {
    if (p.n_frames <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_viterbi_k7f, dim3((unsigned)blocks), dim3(256), 0, st, p);
    return hipGetLastError();
}

} // namespace ofdm
