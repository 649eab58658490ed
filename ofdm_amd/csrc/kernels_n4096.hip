// kernels_n4096.hip -- the shape-specialised N = 4096 kernels (config 5), FFT as 64 x 64 in the k_demod64 layout (kernels_n64.hip):
//   k_demod4096     RX demod: regular symbol streams, and the data symbols of frames after timing
//   k_tx4096        continuous-stream TX
//   k_txframe4096   encode in one pass over HBM
#include "device_common.hpp"
#include "kernels.hpp"

namespace ofdm {

// ---------------------------------------------------------------------------------------------------------------
// k_demod4096: RX demod of N = 4096 symbols (BASELINE config 5) as 64 x 64: one 512-thread workgroup per symbol.
//     X[c + 64 d] = sum_b W64^(b d) * [ W4096^(b c) * sum_a x[64 a + b] W64^(a c) ]
//   stage A  wavefront w, 8-lane group s: the FFT64 over a for column b = 8 w + s, straight from HBM in the Stockham
//            pattern (the next symbol's loads are already in flight), in the k_demod64 layout: wave-local, no barrier;
//   twiddle  W4096^(b c): eight loop-invariant registers per lane;
//   transpose through LDS ([c][b], one barrier);
//   stage B  the FFT64 over b for row c = 8 w + s, again wave-local;
//   epilogue equalise, mean pilot angle over the 256 pilots (wave sums + one LDS step), hard decisions, LSB-first packing
//            through LDS, dword stores -- the same arithmetic as k_sym<4096, M_DEMOD>.
// Four radix-8 butterflies per point like the generic kernel, but ONE workgroup-wide exchange instead of three, four
// barriers per symbol instead of nine, and ~110 VGPRs (two workgroups per CU instead of one).
struct Big4096Params {
    const float2 *in;
    long long frame_stride;
    long long total;          // symbols
    int syms_per_frame, first_symbol;
    long long step_f;         // frames / symbols that one grid step (gridDim.x symbols) advances: no division in the loop
    int step_k;
    const float2 *tw;         // exp(-2 pi i m / 4096), m < 4096
    const float2 *hk;         // optional channel, hk_stride = 0 (shared) or 4096 (per frame)
    long long hk_stride;
    unsigned char *out;
    long long out_stride;
    int bps, guard;
    // FRAME = true (the decode chain after timing, src/receiver.rs:20-83): per-frame start of the trimmed frame, CFO and live
    // symbol count; samples at or past frame_len read as zero (pad_chunk, receiver.rs:203-210)
    const int32_t *offset;
    const double *f_delta;
    const int32_t *nsym_frame;
    long long frame_len;
};

template <int BPS, bool GUARD, bool FRAME>
__global__ __launch_bounds__(512, 4) void k_demod4096(Big4096Params p) { // 4 waves per SIMD = two workgroups per CU: never more than 128 VGPRs
    constexpr int N = 4096, S = 5120, CP = 1024, TS = 72, SLAB = 8 * 72;
    constexpr int ND = GUARD ? 48 * 64 : N;
    constexpr int IMG_DW = ND * BPS / 32;                        // packed bytes of one symbol, in dwords (<= 1024)
    extern __shared__ __align__(16) unsigned char smem[];
    cf *slab_all = reinterpret_cast<cf *>(smem);                 // [8 waves][8 x 72] FFT64 transpose slabs (stages A and B)
    cf *T = slab_all + 8 * SLAB;                                 // [64][72]  Z[c][b]
    unsigned *img = reinterpret_cast<unsigned *>(T + 64 * TS);   // [IMG_DW] the symbol's packed output image
    float *red = reinterpret_cast<float *>(img + 1024);          // [8] wave sums of the pilot angles

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int s = lane >> 3, t = lane & 7;
    const int col = 8 * wave + s;                 // b in stage A, c in stage B
    cf *buf = slab_all + wave * SLAB + s * 72;
    const int wr = swz(8 * t);

    // W64^(r t), r = 1 .. 7, read from a 56-entry LDS table at use: as fourteen loop-invariant registers they pushed the kernel over its
    // 128 VGPRs, and a spilled register comes back through scratch -- a VMEM load, in order behind the next symbol's prefetch, so that every
    // reload waited for the prefetch (round-5 ISA scan: 3 to 10 spilled registers in every instantiation, each reloaded right after a barrier)
    cf *wtab = reinterpret_cast<cf *>(reinterpret_cast<unsigned char *>(red) + 64 + 256);   // [8][7], behind the pilot sums and the frame-mode offset table
    if (tid < 56) wtab[tid] = p.tw[64 * (tid % 7 + 1) * (tid / 7)];
    __syncthreads();
    const cf *w = wtab + 7 * t;
    cf z[8];                                      // W4096^(b c), c = t + 8 q
#pragma unroll
    for (int q = 0; q < 8; ++q) z[q] = p.tw[col * (t + 8 * q)];
    // bit offset of bin c + 64 d (d = t + 8 q) in the image, -1 = not a data bin.  Stream mode keeps the eight of them in registers;
    // frame mode (offsets, CFO phasors, the zero-fill masks of the branch-free fetch on top) spilled 8-17 registers at 128 VGPRs, so
    // there the offset is rebuilt from a 64-entry LDS table of its column-independent part (a spill reload waits for the prefetch)
    int boff_r[8];
    int *btab = reinterpret_cast<int *>(red + 16); // [64] (FRAME only; red + 8 is the spare dword img[1024 + 8] of the packing below)
    if (FRAME) {
        if (tid < 64) { const int d = (tid & 7) + 8 * (tid >> 3); btab[tid] = carrier_class64(d, GUARD) == 0 ? (GUARD ? data_classes_below64(d) : d) * 64 * BPS : -1; }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int d = t + 8 * q;
        boff_r[q] = FRAME ? 0 : (carrier_class64(d, GUARD) == 0 ? ((GUARD ? data_classes_below64(d) : d) * 64 + col) * BPS : -1);
    }
    auto boff = [&](int q) -> int {
        if (!FRAME) return boff_r[q];
        const int b0 = btab[8 * q + t];
        return b0 < 0 ? -1 : b0 + col * BPS;
    };
    constexpr int nbytes = ND * BPS / 8;

    // (frame, symbol) of the symbol one step ahead (the prefetch); advanced by the host's per-step increments -- the two 64-bit
    // divisions per symbol this replaces were a third of the loop's instruction stream (408 of 1214, all scalar)
    long long fn = blockIdx.x / p.syms_per_frame;
    int kn = (int)(blockIdx.x - fn * p.syms_per_frame);
    // Loads are issued without a branch (a load under `if (in range)` is followed by s_waitcnt vmcnt(0) at the join, i.e. is
    // synchronous): out-of-range elements read the twiddle table instead and are zeroed when they leave the prefetch registers.
    // room = samples from this lane's first one to the end of the capture (FRAME), 0 past the batch.
    // FRAME: the frame's scalars (trimmed start, live symbols, CFO) are requested a step ahead (FS tq) and taken where the next
    // prefetch starts: read where they were used, each was followed by s_waitcnt vmcnt(0) -- the start offset ahead of the sample
    // prefetch, the symbol count right behind it (draining it), the CFO, then the channel in four more round trips (round-5 ISA scan).
    struct FS { int off, ns; double fd; };
    const int vzero = pinned(0);   // keeps the workgroup-uniform scalar loads vector loads (as scalar loads they are waited for where they are issued)
    auto load_scalars = [&](bool in, long long fr_) -> FS {
        const long long fr = (in ? fr_ : 0) + vzero;
        FS r;
        r.off = p.offset ? p.offset[fr] : 0;
        r.ns = p.nsym_frame ? p.nsym_frame[fr] : p.syms_per_frame;
        r.fd = p.f_delta ? p.f_delta[fr] : 0.0;
        return r;
    };
    auto fetch = [&](long long sg, long long fr_, int kk, long long off_, cf *dst, int &room) {
        const bool in = sg < p.total;
        const long long fr = in ? fr_ : 0;
        const long long off = FRAME ? off_ : 0;
        const long long n0 = off + (long long)(p.first_symbol + kk) * S + CP + col;
        const cf *src = p.in + fr * p.frame_stride + n0;
        long long rm = FRAME ? p.frame_len - n0 : (long long)N;
        rm = in ? rm : 0;
        room = (int)(rm < 0 ? 0 : (rm > N ? N : rm));
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int i = 64 * (t + 8 * m);
            const cf *a = FRAME ? (i < room ? src + i : p.tw + i) : (in ? src : p.tw) + i; // p.tw: N mapped entries
            dst[m] = *a;
        }
    };
    // The image of symbol j is stored to HBM in iteration j + 1, behind that iteration's FIRST barrier (which is what makes the
    // image complete: no barrier of its own) and long before the next wait for prefetched samples: loads and stores share the
    // in-order VM counter, so stores issued just before a wait-for-loads would be waited for as well.
    // image -> global, and clear it for the next symbol (same thread, same dwords).  Straight-line code: written as a loop over the
    // dwords, the compiler put s_waitcnt vmcnt(0) in front of it -- i.e. the whole workgroup waited here, once per symbol, for the NEXT
    // symbol's samples, which had been requested a few hundred instructions earlier (round-5 ISA scan).  IMG_DW is a multiple of 4 and at
    // most 1024: with 16-byte aligned rows one predicated 16-byte store per thread, else at most two dword stores.
    // (Whole-byte / nibble fields are written with plain stores, every dword of the image by exactly one lane: nothing to clear there;
    //  only the atomic-OR packing of 1-, 2- and 6-bit fields needs a zeroed image -- and a zero 4-vector was one more register than the
    //  kernel has: it came back from scratch, a VMEM load the prefetch had to be waited for behind.)
    const bool wide_out = ((reinterpret_cast<uintptr_t>(p.out) | (uintptr_t)p.out_stride) & 15) == 0;   // (nbytes is a multiple of 16)
    constexpr bool CLEAR = !(BPS == 8 || BPS == 4);
    auto flush = [&](unsigned *dst) {
        if (wide_out) {
            if (tid < IMG_DW / 4) {
                unsigned *i1 = img + 4 * tid;
                reinterpret_cast<uint4 *>(dst)[tid] = *reinterpret_cast<const uint4 *>(i1);
                if (CLEAR) { i1[0] = 0u; i1[1] = 0u; i1[2] = 0u; i1[3] = 0u; }
            }
        } else {
            if (tid < IMG_DW) { dst[tid] = img[tid]; if (CLEAR) img[tid] = 0u; }
            if (IMG_DW > 512 && tid + 512 < IMG_DW) { dst[tid + 512] = img[tid + 512]; if (CLEAR) img[tid + 512] = 0u; }
        }
    };
    for (int i = tid; i < IMG_DW; i += 512) img[i] = 0u;
    cf pre[8];
    int room_pre = 0;
    auto advance = [&](long long &ff, int &kk) { ff += p.step_f; kk += p.step_k; if (kk >= p.syms_per_frame) { kk -= p.syms_per_frame; ++ff; } };
    // positions: the symbol being transformed (f0, k0), the one whose samples are prefetched (fn, kn), the one whose scalars are (f2, k2)
    long long f0 = fn, f2; int k0 = kn, k2;
    advance(fn, kn);
    f2 = fn; k2 = kn; advance(f2, k2);
    FS tq = FS{0, 0, 0.0};
    int ns_cur = 0; double fd_cur = 0.0;
    {
        FS s0 = FS{0, 0, 0.0};
        if (FRAME) s0 = load_scalars(blockIdx.x < p.total, f0);
        fetch(blockIdx.x, f0, k0, s0.off, pre, room_pre);
        ns_cur = __builtin_amdgcn_readfirstlane(s0.ns);
        fd_cur = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(s0.fd)), __builtin_amdgcn_readfirstlane(__double2loint(s0.fd)));
        if (FRAME) tq = load_scalars((long long)blockIdx.x + gridDim.x < p.total, fn);
    }
    unsigned *pending = nullptr; // where the image currently in LDS belongs

    for (long long sg = blockIdx.x; sg < p.total; sg += gridDim.x) {
        const long long f = f0;
        const int k = k0;
        cf v[8];
#pragma unroll
        for (int m = 0; m < 8; ++m) v[m] = (!FRAME || 64 * (t + 8 * m) < room_pre) ? pre[m] : make_float2(0.f, 0.f);
        // the next symbol's scalars (requested a step ago, right behind this symbol's samples): workgroup-uniform -> SGPRs
        const int off_n = FRAME ? __builtin_amdgcn_readfirstlane(tq.off) : 0;
        const int ns_n = FRAME ? __builtin_amdgcn_readfirstlane(tq.ns) : 0;
        const double fd_n = FRAME ? __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(tq.fd)), __builtin_amdgcn_readfirstlane(__double2loint(tq.fd))) : 0.0;
        if (!FRAME) fetch(sg + gridDim.x, fn, kn, 0, pre, room_pre);   // stream mode: nothing else is loaded, the prefetch goes out first
        bool live = true;
        if (FRAME) {
            if (k >= ns_cur) live = false; // fewer symbols in this frame: nothing is written (workgroup-uniform)
            if (!live) {
#pragma unroll
                for (int m = 0; m < 8; ++m) v[m] = make_float2(0.f, 0.f);
            } else if (p.f_delta) { // CFO derotation, sample ids count from the trimmed start (receiver.rs:44-50); phase reduced in f64
                const double turns = fd_cur * 0.15915494309189533577;
                cf ph = cfo_phasor(turns, (long long)(p.first_symbol + k) * S + CP + col + 64 * t);
                const cf st = cfo_phasor(turns, 512);
#pragma unroll
                for (int m = 0; m < 8; ++m) { v[m] = cmul(v[m], ph); ph = cmul(ph, st); }
            }
        }
        unsigned *const mine = live ? reinterpret_cast<unsigned *>(p.out + f * p.out_stride + (long long)k * nbytes) : nullptr;
        // ---- stage A: FFT64 over a (wave-local)
        bfly8<false>(v);
#pragma unroll
        for (int r = 0; r < 8; ++r) buf[wr ^ r] = v[r];
#pragma unroll
        for (int m = 0; m < 8; ++m) v[m] = buf[8 * m + (t ^ m)];
#pragma unroll
        for (int r = 1; r < 8; ++r) v[r] = cmul(v[r], w[r - 1]);
        bfly8<false>(v);
        // v[q] = Y_b[c = t + 8 q]; twiddle and transpose
#pragma unroll
        for (int q = 0; q < 8; ++q) T[(t + 8 * q) * TS + (col ^ (t & 6))] = cmul(v[q], z[q]); // column XOR-swizzled by the row: conflict-free both ways
        __syncthreads(); // T complete; the PREVIOUS symbol's image complete (two barriers per symbol, not three: see below)
        if (pending) flush(pending); // ... so it leaves for HBM here, cleared for this symbol's fields, which are written after the next barrier
        pending = mine;
        // FRAME: this symbol's channel is requested here and used behind stage B; only THEN does the next symbol's prefetch go out (its
        // registers are free while the channel's are live: no register more than before) -- requested at its use the channel came in four
        // serialized round trips, requested behind the prefetch its wait would drain the prefetch
        cf hkv[8];
        if (FRAME) {
            const cf *h = p.hk ? p.hk + f * p.hk_stride + col : p.tw;
#pragma unroll
            for (int q = 0; q < 8; ++q) hkv[q] = h[64 * (t + 8 * q)];
            __builtin_amdgcn_sched_barrier(0);   // (left alone the scheduler sinks these loads to their use, behind stage B: a round trip in the open)
        }
        // ---- stage B: FFT64 over b for row c = col
#pragma unroll
        for (int m = 0; m < 8; ++m) v[m] = T[col * TS + (t ^ (col & 6)) + 8 * m]; // (t + 8 m) ^ s = (t ^ s) + 8 m for s < 8: offsets stay immediates
        bfly8<false>(v);
#pragma unroll
        for (int r = 0; r < 8; ++r) buf[wr ^ r] = v[r];
#pragma unroll
        for (int m = 0; m < 8; ++m) v[m] = buf[8 * m + (t ^ m)];
#pragma unroll
        for (int r = 1; r < 8; ++r) v[r] = cmul(v[r], w[r - 1]);
        bfly8<false>(v);
        // v[q] = X[col + 64 (t + 8 q)]
        if (p.hk) { // equalise: Y /= H (src/receiver.rs:68-70)
            const cf *h = p.hk + f * p.hk_stride;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const cf hh = FRAME ? hkv[q] : h[col + 64 * (t + 8 * q)];
                const float rn = __builtin_amdgcn_rcpf(hh.x * hh.x + hh.y * hh.y);
                const cf e = cmulc(v[q], hh);
                v[q] = make_float2(e.x * rn, e.y * rn);
            }
        }
        if (FRAME) {   // the next symbol's samples from the start offset that arrived with this symbol's, then the scalars of the one after
            fetch(sg + gridDim.x, fn, kn, off_n, pre, room_pre);
            tq = load_scalars(sg + 2 * (long long)gridDim.x < p.total, f2);
        }
        f0 = fn; k0 = kn; fn = f2; kn = k2; advance(f2, k2);
        ns_cur = ns_n; fd_cur = fd_n;
        cf rot = make_float2(1.f, 0.f);
        if (GUARD) { // decode_block (src/receiver.rs:106-145): mean angle of the 4 x 64 pilots, rotate by -phase
            // pilot classes 6, 25, 39, 58 = (t, q) = (6, 0), (1, 3), (7, 4), (2, 7); other lanes feed (1, 0) -> angle 0
            cf pv = make_float2(1.f, 0.f);
            pv = (t == 6) ? v[0] : pv;
            pv = (t == 1) ? v[3] : pv;
            pv = (t == 7) ? v[4] : pv;
            pv = (t == 2) ? v[7] : pv;
            float a = __ocml_atan2pi_f32(pv.y, pv.x);
#pragma unroll
            for (int sh = 32; sh >= 1; sh >>= 1) a += __shfl_xor(a, sh, 64);
            if (lane == 0) red[wave] = a;
            __syncthreads();
            float tot = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) tot += red[i];
            const float trn = tot * (0.5f / 256.0f); // mean of the 256 pilot angles, in turns -> hardware sin / cos
            rot = make_float2(__builtin_amdgcn_cosf(trn), -__builtin_amdgcn_sinf(trn)); // applied inside the demapper
        }
        // demodulate (src/receiver.rs:147-190) and pack LSB-first (src/utils.rs:30-36).  The fields go into the image behind the pilot
        // barrier, which also orders them after the flush of the previous image above; without guard bands there is no pilot
        // barrier, so one stands here.  No barrier closes the step: the image is read (flushed) only behind the next step's first
        // barrier, T is rewritten only by waves that are past the pilot barrier (every stage-B read of T lies before it), and the
        // pilot sums are rewritten only behind the next step's first barrier.
        if (!GUARD) __syncthreads();
        if (BPS == 8 || BPS == 4) {
            // Whole-byte / nibble fields: the 32 / BPS lane groups s that share a dword (same t, so the same carrier class)
            // merge their fields in registers -- lane ^ 8 by DPP, lane ^ 16 by ds_swizzle, lane ^ 32 by a shuffle -- and ONE
            // lane writes the dword with a plain store: no atomics, no 4-way same-dword serialisation (round-2 ablation on
            // noise input: loads 0.49 ms, + stage A / transpose 0.06, + stage B / pilots 0.19, + demap / packing 0.28, + stores 0.10), and the image needs no clearing
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                // branch-free: rows q in {1, 2, 5, 6} hold data bins in every lane; elsewhere non-data lanes contribute 0 and
                // non-writing lanes store to a spare dword behind the image (exec-mask branches cost more than the stores)
                const bool all_data = !GUARD || q == 1 || q == 2 || q == 5 || q == 6;
                const int bo = boff(q);
                const bool data = live && (all_data || bo >= 0); // a dead symbol writes nothing into the image
                unsigned val = (GUARD ? demap_point_rot(v[q], rot, BPS) : demap_point(v[q], BPS)) << (BPS * (s & (32 / BPS - 1)));
                val = data ? val : 0u;
                val |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)val, 0x128, 0xF, 0xF, true);          // row_ror:8   : s ^ 1 (dpp_i<0x128> written out: as a call the v_or operands swap)
                val |= (unsigned)__builtin_amdgcn_ds_swizzle((int)val, 0x401F);                               // xor 16      : s ^ 2
                if (BPS == 4) val |= (unsigned)__shfl_xor((int)val, 32, 64);                                  // s ^ 4
                img[(data && (s & (32 / BPS - 1)) == 0) ? (bo >> 5) : 1024 + 8] = val;
            }
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) { // OR every field into the image; a dead symbol (k >= nsym_frame[f]) must leave it clear:
                const int bo = boff(q);
                if (live && bo >= 0) { // nothing flushes the image after such a step, and demap_point(0) != 0 for BPS >= 2
                    const unsigned idx = GUARD ? demap_point_rot(v[q], rot, BPS) : demap_point(v[q], BPS);
                    or_field<BPS>(img, bo, idx);
                }
            }
        }
    }
    __syncthreads(); // the last image is complete
    if (pending) flush(pending);
}

// N = 4096 RX demod fast path: regular symbol streams, and the data symbols of frames after timing (per-frame offset, CFO,
// live-symbol count, zero-fill past the capture).  hipErrorNotSupported => caller uses k_sym<4096, M_DEMOD>.
hipError_t run_demod4096(const SymParams &sp, hipStream_t st, int num_cu) {
    if (sp.soft || sp.syms_per_frame <= 0) return hipErrorNotSupported;
    if (sp.in_sym_stride != 5120 || sp.in_skip != 1024) return hipErrorNotSupported;
    const bool frame = sp.offset || sp.f_delta || sp.nsym_frame ||
                       (long long)(sp.first_symbol + sp.syms_per_frame) * 5120 > sp.frame_len; // tail padding needs the bounds checks
    const int nd = sp.guard ? 48 * 64 : 4096;
    if ((nd * sp.bps / 8) % 4 != 0 || (reinterpret_cast<uintptr_t>(sp.out_bytes) & 3) || (sp.out_stride & 3)) return hipErrorNotSupported;
    if (sp.hk && sp.hk_stride != 0 && sp.hk_stride != 4096) return hipErrorNotSupported;
    Big4096Params p;
    p.in = sp.in; p.frame_stride = sp.frame_stride; p.total = sp.n_frames * (long long)sp.syms_per_frame;
    p.syms_per_frame = sp.syms_per_frame; p.first_symbol = sp.first_symbol; p.tw = sp.tw; p.hk = sp.hk; p.hk_stride = sp.hk_stride;
    p.out = sp.out_bytes; p.out_stride = sp.out_stride; p.bps = sp.bps; p.guard = sp.guard;
    p.offset = sp.offset; p.f_delta = sp.f_delta; p.nsym_frame = sp.nsym_frame; p.frame_len = sp.frame_len;
    if (p.total <= 0) return hipSuccess;
    const size_t lds = (size_t)(8 * 8 * 72 + 64 * 72) * sizeof(float2) + 4096 + 64 + 256 + 448; // slabs, T, image, pilot sums + spare dword, frame-mode offset table, stage twiddles
    const long long grid = persistent_grid(p.total, (long long)num_cu * 2, tuning_or_default(sp.tune));
    trace_add(sp.trace, frame ? "k_demod4096<frame>" : "k_demod4096");
    p.step_f = grid / p.syms_per_frame; p.step_k = (int)(grid - p.step_f * p.syms_per_frame);
    // > 64 KB of dynamic LDS: a per-device attribute, so set on every call (one process may drive several GPUs); once per batch
    return with_bps(sp.bps, [&](auto B) { return with_bool(sp.guard != 0, [&](auto G) { return with_bool(frame, [&](auto F) {
        const auto kernel = k_demod4096<decltype(B)::value, decltype(G)::value, decltype(F)::value>;
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(512), lds, st, p);
        return hipGetLastError(); }); }); });
}

// ---------------------------------------------------------------------------------------------------------------
// k_tx4096: modulate + encode_block + prefix_block (src/transmitter.rs:108-181) for a continuous stream of N = 4096
// symbols (BASELINE config 5 TX), the mirror image of k_demod4096:
//     x[c + 64 d] = 1/N sum_b W64^(-b d) * [ W4096^(-b c) * sum_a X[64 a + b] W64^(-a c) ]
// The symbol's bytes are staged in LDS from dwords prefetched one symbol ahead; lane (s, t) of wavefront w builds bins
// 64 (t + 8 m) + b, b = 8 w + s (the carrier class depends on t + 8 m only), runs the inverse FFT64 over a, the twiddle,
// the LDS transpose and the inverse FFT64 over b, and stores samples c + 64 (t + 8 q) behind the cyclic prefix.
struct Tx4096Params {
    const uint8_t *bytes;
    long long n_bytes, n_sym;
    const float2 *tw;   // exp(-2 pi i m / 4096)
    float2 *out;        // n_sym x 5120 samples
    int bps, guard;
};

template <bool GUARD>
__global__ __launch_bounds__(512, 4) void k_tx4096(Tx4096Params p) {
    constexpr int N = 4096, S = 5120, CP = 1024, TS = 72, SLAB = 8 * 72;
    extern __shared__ __align__(16) unsigned char smem[];
    cf *slab_all = reinterpret_cast<cf *>(smem);
    cf *T = slab_all + 8 * SLAB;
    unsigned *sbw = reinterpret_cast<unsigned *>(T + 64 * TS);          // [1024 + 2] the symbol's bytes as dwords
    cf *ptab = reinterpret_cast<cf *>(sbw + 1024 + 4);                  // [256] map_point by raw bit field (transmitter.rs:108-140)

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int s = lane >> 3, t = lane & 7;
    const int col = 8 * wave + s;
    cf *buf = slab_all + wave * SLAB + s * 72;
    const int wr = swz(8 * t);
    if (tid < (1 << p.bps)) ptab[tid] = map_point((unsigned)tid, p.bps);
    const unsigned fmask = (1u << p.bps) - 1u;
    cf w[7];
#pragma unroll
    for (int r = 1; r < 8; ++r) { const cf x = p.tw[64 * r * t]; w[r - 1] = make_float2(x.x, -x.y); }
    cf z[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) { const cf x = p.tw[col * (t + 8 * q)]; z[q] = make_float2(x.x, -x.y); }
    int boff[8]; // bit offset of bin 64 (t + 8 m) + col inside the symbol's stream, -1 = null, -2 = pilot
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int a = t + 8 * m, cls = carrier_class64(a, GUARD);
        boff[m] = cls == 0 ? ((GUARD ? data_classes_below64(a) : a) * 64 + col) * p.bps : (cls == 2 ? -2 : -1);
    }
    const int nd = GUARD ? 48 * 64 : N;
    const int sym_bytes = nd * p.bps / 8;   // <= 4096, multiple of 4 (checked by the launcher)
    const bool aligned = (reinterpret_cast<uintptr_t>(p.bytes) & 3) == 0;
    // stream bytes of symbol sg, two dwords per thread: issued without a branch (paydw_issue), settled where they are used
    const bool want0 = 4 * tid < sym_bytes, want1 = 4 * (tid + 512) < sym_bytes;
    auto fetch = [&](long long sg, unsigned &d0, unsigned &d1) {
        const long long base = sg * sym_bytes;
        const bool in = sg < p.n_sym;
        d0 = paydw_issue(p.bytes, base + 4 * tid, p.n_bytes, in && want0, aligned, p.tw);
        d1 = paydw_issue(p.bytes, base + 4 * (tid + 512), p.n_bytes, in && want1, aligned, p.tw);
    };
    auto settle = [&](long long sg, unsigned d0, unsigned d1) {
        const long long base = sg * sym_bytes;
        const bool in = sg < p.n_sym;
        sbw[tid] = paydw_settle(d0, p.bytes, base + 4 * tid, p.n_bytes, in && want0, aligned);
        sbw[tid + 512] = paydw_settle(d1, p.bytes, base + 4 * (tid + 512), p.n_bytes, in && want1, aligned);
    };
    // The bytes of symbol j+1 are taken out of the prefetch registers (and symbol j+2's loads issued) BEFORE symbol j's
    // samples are stored: loads and stores share the in-order VM counter, so a wait for prefetched loads placed after the
    // stores would wait for the stores as well.
    unsigned d0, d1;
    fetch(blockIdx.x, d0, d1);
    settle(blockIdx.x, d0, d1);
    if (tid < 2) sbw[1024 + tid] = 0u; // slack for the two-byte window
    fetch((long long)blockIdx.x + gridDim.x, d0, d1);
    __syncthreads();

    for (long long sg = blockIdx.x; sg < p.n_sym; sg += gridDim.x) {
        long long left = p.n_bytes - sg * sym_bytes;             // stream bytes that belong to this symbol
        left = left < 0 ? 0 : (left < sym_bytes ? left : sym_bytes);
        const int live_bits = (int)(((unsigned)left * 8u + (unsigned)p.bps - 1u) / (unsigned)p.bps) * p.bps; // fields that carry stream bits (left <= 4096); the rest are 0
        cf v[8];
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            // constellation points from an LDS table filled with map_point itself (bit-identical values) instead of ~20
            // instructions of Gray decoding per axis (round-2 ablation: 0.21 of 1.09 ms); branch-free
            v[m] = tx_point<true>(sbw, ptab, boff[m], live_bits, fmask);
        }
        bfly8<true>(v);
#pragma unroll
        for (int r = 0; r < 8; ++r) buf[wr ^ r] = v[r];
#pragma unroll
        for (int m = 0; m < 8; ++m) v[m] = buf[8 * m + (t ^ m)];
#pragma unroll
        for (int r = 1; r < 8; ++r) v[r] = cmul(v[r], w[r - 1]);
        bfly8<true>(v);
#pragma unroll
        for (int q = 0; q < 8; ++q) T[(t + 8 * q) * TS + (col ^ (t & 6))] = cmul(v[q], z[q]); // column XOR-swizzled by the row: conflict-free both ways
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 8; ++m) v[m] = T[col * TS + (t ^ (col & 6)) + 8 * m]; // (t + 8 m) ^ s = (t ^ s) + 8 m for s < 8: offsets stay immediates
        bfly8<true>(v);
#pragma unroll
        for (int r = 0; r < 8; ++r) buf[wr ^ r] = v[r];
#pragma unroll
        for (int m = 0; m < 8; ++m) v[m] = buf[8 * m + (t ^ m)];
#pragma unroll
        for (int r = 1; r < 8; ++r) v[r] = cmul(v[r], w[r - 1]);
        bfly8<true>(v);
        // v[q] = N x[col + 64 (t + 8 q)]; prefix_block: out = [x[N - CP .. N), x[0 .. N)]
        settle(sg + gridDim.x, d0, d1); // next symbol's bytes (every wavefront left the mapping stage two barriers ago)
        fetch(sg + 2 * (long long)gridDim.x, d0, d1);
        // transpose once more through T ([n >> 6][n & 63], the conflict-free layout of the first transpose) so that every
        // store is a full 16 bytes per lane and 1 KiB per wavefront
        __syncthreads(); // every wavefront has read its stage-B inputs out of T
#pragma unroll
        for (int q = 0; q < 8; ++q) T[(t + 8 * q) * TS + (col ^ (t & 6))] = make_float2(v[q].x * (1.0f / N), v[q].y * (1.0f / N));
        __syncthreads();
        {
            float4 *dst4 = reinterpret_cast<float4 *>(p.out + sg * S);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = tid + 512 * j, n = 2 * i;                      // sample pair (n, n + 1)
                const float4 y = *reinterpret_cast<const float4 *>(T + (n >> 6) * TS + ((n & 63) ^ ((n >> 6) & 6))); // an even XOR keeps the pair adjacent
                dst4[(CP >> 1) + i] = y;
                if (j == 3) dst4[i - ((N - CP) >> 1)] = y;                   // n >= N - CP: the cyclic prefix
            }
        }
        __syncthreads(); // sbw / T are reused by the next symbol
    }
}

// Continuous-stream TX for N = 4096.  hipErrorNotSupported => caller uses k_sym<4096, M_TX>.
hipError_t run_tx4096(const SymParams &sp, hipStream_t st, int num_cu) {
    if (sp.tx_raw_total < 0 || sp.syms_per_frame != 1 || sp.payload_len) return hipErrorNotSupported;
    const int nd = sp.guard ? 48 * 64 : 4096;
    const int sym_bytes = nd * sp.bps / 8;
    if ((sym_bytes & 3) || sp.payload_stride != sym_bytes || sp.out_stride_s != 5120) return hipErrorNotSupported;
    if (reinterpret_cast<uintptr_t>(sp.out) & 15) return hipErrorNotSupported; // 16-byte stores
    if (sp.n_frames <= 0) return hipSuccess;
    Tx4096Params p;
    p.bytes = sp.payload; p.n_bytes = sp.tx_raw_total; p.n_sym = sp.n_frames; p.tw = sp.tw; p.out = sp.out; p.bps = sp.bps; p.guard = sp.guard;
    const size_t lds = (size_t)(8 * 8 * 72 + 64 * 72) * sizeof(float2) + 4096 + 16 + 256 * sizeof(float2); // slabs, T, byte window + slack, point table
    const long long grid = persistent_grid(p.n_sym, (long long)num_cu * 2, tuning_or_default(sp.tune));
    return with_bool(sp.guard != 0, [&](auto G) {
        const auto kernel = k_tx4096<decltype(G)::value>;
        // > 64 KB of dynamic LDS: per device, so set on every call (one process may drive several GPUs); once per batch
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        trace_add(sp.trace, "k_tx4096");
        hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(512), lds, st, p);
        return hipGetLastError(); });
}

// ---------------------------------------------------------------------------------------------------------------
// k_txframe4096: encode (src/transmitter.rs:11-58) for N = 4096 in ONE pass over HBM, the frame-level sibling of k_tx4096 and
// the R = 64 member of k_txframe_mid's scheme (kernels_mid.hip): one 512-thread workgroup per frame builds the frame's data
// symbols TWICE -- pass 0 only for the signed maximum normalize needs (transmitter.rs:184-188), pass 1 to store them divided
// by it -- instead of writing, reading back and rewriting them (k_sym<4096, M_TX> + k_tx_finish: 24 B of traffic per sample).
// One instance of the symbol builder, the pass is a uniform branch around the two epilogues.
struct TxFrame4096Params {
    const uint8_t *payload;
    long long payload_stride;
    const int32_t *payload_len;
    int payload_bytes;
    long long n_frames;
    int D;               // data symbols per frame
    const float2 *tw;    // exp(-2 pi i m / 4096)
    const float2 *header; // 10 S samples
    float header_max;
    float2 *out;
    long long out_stride; // samples
    int bps;
    int optimistic;      // as k_txframe_mid: symbols leave divided by the header maximum; a frame that exceeds it is built again
};

template <bool GUARD>
__global__ __launch_bounds__(512, 4) void k_txframe4096(TxFrame4096Params p) {
    constexpr int N = 4096, S = 5120, CP = 1024, TS = 72, SLAB = 8 * 72;
    extern __shared__ __align__(16) unsigned char smem[];
    cf *slab_all = reinterpret_cast<cf *>(smem);
    cf *T = slab_all + 8 * SLAB;
    unsigned *sbw = reinterpret_cast<unsigned *>(T + 64 * TS);          // [1024 + 4] the symbol's bytes as dwords + slack
    cf *ptab = reinterpret_cast<cf *>(sbw + 1024 + 4);                  // [256] map_point by raw bit field
    unsigned *fmax = reinterpret_cast<unsigned *>(ptab + 256);          // [1] max(0, re, im) of the frame's data symbols, float bits

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int s = lane >> 3, t = lane & 7;
    const int col = 8 * wave + s;
    cf *buf = slab_all + wave * SLAB + s * 72;
    const int wr = swz(8 * t);
    if (tid < (1 << p.bps)) ptab[tid] = map_point((unsigned)tid, p.bps);
    if (tid < 4) sbw[1024 + tid] = 0u;
    const unsigned fmask = (1u << p.bps) - 1u;
    cf w[7];
#pragma unroll
    for (int r = 1; r < 8; ++r) { const cf x = p.tw[64 * r * t]; w[r - 1] = make_float2(x.x, -x.y); }
    cf z[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) { const cf x = p.tw[col * (t + 8 * q)]; z[q] = make_float2(x.x, -x.y); }
    int boff[8]; // bit offset of bin 64 (t + 8 m) + col inside the symbol's stream, -1 = null, -2 = pilot
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int a = t + 8 * m, cls = carrier_class64(a, GUARD);
        boff[m] = cls == 0 ? ((GUARD ? data_classes_below64(a) : a) * 64 + col) * p.bps : (cls == 2 ? -2 : -1);
    }
    const int nd = GUARD ? 48 * 64 : N;
    const int sym_bytes = nd * p.bps / 8;   // <= 4096, a multiple of 4
    const bool aligned = ((reinterpret_cast<uintptr_t>(p.payload) | (uintptr_t)p.payload_stride) & 3) == 0;
    // The stream bytes of symbol (f, k) -- two dwords per lane -- and the frame's length are REQUESTED one symbol ahead and taken out of
    // the registers when the symbol is built (paydw_issue / paydw_settle, as k_txframe_mid): read where they are used they cost a
    // dependent round trip to HBM per symbol.  The barriers of this kernel are LDS-only (lds_barrier) so that the request stays in flight.
    struct Pre { unsigned d0, d1; int len_raw; };
    auto issue_sym = [&](bool valid, long long f, int k, Pre &pr) {
        const long long fc = valid ? f : 0;
        const uint8_t *pay = p.payload + fc * p.payload_stride;
        const long long by0 = (long long)k * sym_bytes + 4 * tid - 16, by1 = by0 + 2048;   // payload byte of this lane's two dwords
        pr.d0 = paydw_issue(pay, by0, p.payload_bytes, valid && 4 * tid < sym_bytes, aligned, p.tw);
        pr.d1 = paydw_issue(pay, by1, p.payload_bytes, valid && 4 * (tid + 512) < sym_bytes, aligned, p.tw);
        pr.len_raw = p.payload_len ? p.payload_len[fc] : p.payload_bytes;
    };
    Pre pre;
    issue_sym(blockIdx.x < p.n_frames, blockIdx.x, 0, pre);

    for (long long f = blockIdx.x; f < p.n_frames; f += gridDim.x) {
        if (tid == 0) *fmax = 0u;
        const uint8_t *pay = p.payload + f * p.payload_stride;
        cf *row = p.out + f * p.out_stride;
        // Optimistic scheme (kernels_mid.hip, k_txframe_mid): pass 0 builds every symbol once, notes its maximum and stores it
        // divided by the header maximum; pass 1 -- every symbol again, divided by the true maximum -- runs only for a frame whose data
        // exceeded the header (crafted payloads).  Without p.optimistic pass 0 only forms the maximum (the round-4 scheme, the A/B).
        const bool opt = p.optimistic != 0;
        for (int pass = 0; pass < 2; ++pass) {
            if (pass == 1) { // header blocks (src/transmitter.rs:22-34), divided by the frame maximum like the data
                lds_barrier();
                const float inv = 1.0f / fmaxf(p.header_max, __uint_as_float(*fmax));
                float4 *dst4 = reinterpret_cast<float4 *>(row);
                const float4 *h4 = reinterpret_cast<const float4 *>(p.header);
                // four table reads in flight per lane, then their four stores; unconditional reads from a clamped index
                for (int i0 = tid; i0 < 5 * S; i0 += 4 * 512) {
                    float4 h[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) { const int i = i0 + 512 * j; h[j] = h4[i < 5 * S ? i : 5 * S - 1]; }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int i = i0 + 512 * j;
                        if (i < 5 * S) dst4[i] = make_float4(h[j].x * inv, h[j].y * inv, h[j].z * inv, h[j].w * inv);
                    }
                }
                if (opt && !(__uint_as_float(*fmax) > p.header_max)) break;
            }
            for (int k = 0; k < p.D; ++k) {
                const long long sb0 = (long long)k * sym_bytes;
                Pre cur;
                if (opt && pass == 1) issue_sym(true, f, k, cur);   // the rare rebuild asks where it uses; `pre` keeps the next frame's
                else {
                    cur = pre;
                    // the next item: the next symbol, the first symbol of pass 1 (two-pass scheme), or the first of the workgroup's next frame
                    if (k + 1 < p.D) issue_sym(true, f, k + 1, pre);
                    else if (pass == 0 && !opt) issue_sym(true, f, 0, pre);
                    else issue_sym(f + gridDim.x < p.n_frames, f + gridDim.x, 0, pre);
                }
                const long long len = row_len(cur.len_raw, p.payload_bytes);
                // stream bytes of a frame: [16-byte little-endian length | payload | zeros] (src/packets/mod.rs:20-32)
                auto word = [&](unsigned raw, long long sb, bool want) -> unsigned {
                    if (!want) return 0u;
                    if (sb < 16) return sb < 8 ? (unsigned)((unsigned long long)len >> (8 * sb)) : 0u;
                    return paydw_settle(raw, pay, sb - 16, len, true, aligned);
                };
                sbw[tid] = word(cur.d0, sb0 + 4 * tid, 4 * tid < sym_bytes);
                sbw[tid + 512] = word(cur.d1, sb0 + 4 * (tid + 512), 4 * (tid + 512) < sym_bytes);
                lds_barrier(); // the byte window is complete (and, first time round, fmax / ptab are set)
                long long left = 16 + len - sb0;                     // stream bytes that belong to this symbol
                left = left < 0 ? 0 : (left < sym_bytes ? left : sym_bytes);
                const int live_bits = (int)(((unsigned)left * 8u + (unsigned)p.bps - 1u) / (unsigned)p.bps) * p.bps;
                cf v[8];
#pragma unroll
                for (int m = 0; m < 8; ++m) v[m] = tx_point<true>(sbw, ptab, boff[m], live_bits, fmask);
                bfly8<true>(v);
#pragma unroll
                for (int r = 0; r < 8; ++r) buf[wr ^ r] = v[r];
#pragma unroll
                for (int m = 0; m < 8; ++m) v[m] = buf[8 * m + (t ^ m)];
#pragma unroll
                for (int r = 1; r < 8; ++r) v[r] = cmul(v[r], w[r - 1]);
                bfly8<true>(v);
#pragma unroll
                for (int q = 0; q < 8; ++q) T[(t + 8 * q) * TS + (col ^ (t & 6))] = cmul(v[q], z[q]);
                lds_barrier();
#pragma unroll
                for (int m = 0; m < 8; ++m) v[m] = T[col * TS + (t ^ (col & 6)) + 8 * m];
                bfly8<true>(v);
#pragma unroll
                for (int r = 0; r < 8; ++r) buf[wr ^ r] = v[r];
#pragma unroll
                for (int m = 0; m < 8; ++m) v[m] = buf[8 * m + (t ^ m)];
#pragma unroll
                for (int r = 1; r < 8; ++r) v[r] = cmul(v[r], w[r - 1]);
                bfly8<true>(v);
                // v[q] = N x[col + 64 (t + 8 q)]
                if (pass == 0) {
                    float mine = 0.f;   // max first, one scaling behind it (x -> x / N is monotone: the same bits), three-operand maxima
#pragma unroll
                    for (int q = 0; q < 8; ++q) mine = __builtin_fmaxf(mine, __builtin_fmaxf(v[q].x, v[q].y));
                    mine *= 1.0f / N;
#pragma unroll
                    for (int sh = 32; sh >= 1; sh >>= 1) mine = fmaxf(mine, __shfl_xor(mine, sh, 64));
                    if (lane == 0) atomicMax(fmax, __float_as_uint(mine));
                    if (!opt) {
                        lds_barrier(); // every wavefront has read its stage-B inputs out of T; the byte window is free
                        continue;
                    }
                }
                // one division, then multiplies (<= 1 ulp)
                const float sc = (1.0f / N) / (pass == 0 ? p.header_max : fmaxf(p.header_max, __uint_as_float(*fmax)));
                lds_barrier(); // every wavefront has read its stage-B inputs out of T
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    T[(t + 8 * q) * TS + (col ^ (t & 6))] = make_float2(v[q].x * sc, v[q].y * sc);
                lds_barrier();
                {   // prefix_block: out = [x[N - CP .. N), x[0 .. N)], 16 bytes per lane
                    float4 *dst4 = reinterpret_cast<float4 *>(row + (long long)(10 + k) * S);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int i = tid + 512 * j, n = 2 * i;
                        const float4 y = *reinterpret_cast<const float4 *>(T + (n >> 6) * TS + ((n & 63) ^ ((n >> 6) & 6)));
                        dst4[(CP >> 1) + i] = y;
                        if (j == 3) dst4[i - ((N - CP) >> 1)] = y;
                    }
                }
                lds_barrier(); // the byte window / T are reused by the next symbol
            }
        }
        lds_barrier(); // fmax is reset for the next frame
    }
}

// encode for N = 4096 in one pass.  hipErrorNotSupported => caller runs k_sym<4096, M_TX> + k_tx_finish.
hipError_t run_txframe4096(const SymParams &sp, const float2 *header, float header_max, hipStream_t st, int num_cu) {
    if (sp.tx_raw_total >= 0 || sp.syms_per_frame <= 0) return hipErrorNotSupported;
    if ((reinterpret_cast<uintptr_t>(sp.out) & 15) || (sp.out_stride_s & 1)) return hipErrorNotSupported;
    const int nd = sp.guard ? 48 * 64 : 4096;
    if ((nd * sp.bps / 8) & 3) return hipErrorNotSupported;
    if (sp.n_frames <= 0) return hipSuccess;
    TxFrame4096Params p;
    p.payload = sp.payload; p.payload_stride = sp.payload_stride; p.payload_len = sp.payload_len; p.payload_bytes = sp.payload_bytes;
    p.n_frames = sp.n_frames; p.D = sp.syms_per_frame; p.tw = sp.tw; p.header = header; p.header_max = header_max;
    p.out = sp.out; p.out_stride = sp.out_stride_s; p.bps = sp.bps;
    p.optimistic = tuning_or_default(sp.tune).no_txframe_optimistic ? 0 : 1;
    const size_t lds = (size_t)(8 * 8 * 72 + 64 * 72) * sizeof(float2) + 4096 + 16 + 256 * sizeof(float2) + 16;
    const long long grid = persistent_grid(p.n_frames, (long long)num_cu * 2, tuning_or_default(sp.tune));
    return with_bool(sp.guard != 0, [&](auto G) {
        const auto kernel = k_txframe4096<decltype(G)::value>;
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        trace_add(sp.trace, "k_txframe4096");
        hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(512), lds, st, p);
        return hipGetLastError(); });
}

} // namespace ofdm
