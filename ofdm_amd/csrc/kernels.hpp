// kernels.hpp -- host-visible launch interface of the HIP kernels (internal to libofdm_hip.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include <mutex>

#ifndef OFDM_PROFILE_BUILD
#define OFDM_PROFILE_BUILD 0 // 1 (ofdm_amd/build.py, profile=True): libofdm_hip_profile.so with the ablation / section-timing branches
#endif

namespace ofdm {

// The `debug` branches of the kernels (early exits, s_memtime section ticks) are compiled only into the profile build.
constexpr bool kProfile = OFDM_PROFILE_BUILD != 0;

// Per-context tuning (ofdm_set_tuning): A/B switches between kernel families, grid shapes and the tests' grid cap.  The
// library reads no environment variable; a host that wants one maps it onto these keys itself (tools/tune_env.py).
struct Tuning {
    int no_sc80 = 0;               // L = 80, W = 240: the round-4 f32 filter pair (k_sc_cf<128,first> + k_sc_cf<256,list>) instead of the exact streaming detector k_sc80 (A/B)
    int sc80_depth = 2;            // k_sc80: steps between the last read of a ring piece and its refill (1: 9 - 10 KiB in flight per wavefront, 2: 7)
    int no_sc_stream = 0;          // L = 160 .. 1280: k_scb_chunks + k_scb_fine / k_sc_tile instead of the streaming detector
    int no_sc_big = 0;             // long-period Schmidl-Cox through k_sc_tile instead of k_scb_chunks + k_scb_fine
    int no_fast64 = 0, no_demod4096 = 0, no_mid_kernels = 0, no_rxframe1024 = 0, no_txframe64 = 0; // take the generic k_sym
    int no_rx1024_finish = 0;      // k_rxframe1024 writes raw bytes and k_rx_finish runs as its own launch
    int no_rxframe64_split = 0;    // k_rxframe64 as ONE kernel with both frame bodies (three waves per SIMD) instead of the common-body / cut-body pair (A/B)
    long long grid_cap = 0;        // > 0: caps every persistent grid (test hook: many steps per workgroup on a small batch)
    int tx_waves = 16;             // k_txframe64: wavefronts per CU
    int txframe_keep_steps = 1;    // k_txframe_mid: 1 = frames whose data symbols fit ONE workgroup step (<= 32 / R symbols) are built once, their points kept in registers until the maximum is known; 0 = always twice
    int no_txframe_optimistic = 0; // k_txframe_mid / k_txframe4096, frames of more than one step: 1 = the round-4 scheme (every symbol built twice: once for the frame maximum, once to be stored); 0 = symbols leave divided by the header maximum while the frame maximum forms, a round is rebuilt only if a frame exceeds it
    int txframe_rewrite = 0;       // k_txframe_mid, frames of more than one step: 1 = build every symbol ONCE -- unnormalised samples out, then a rescale sweep over what
                                   // was just written (L2 / memory-side cache) -- instead of building every symbol twice
    int sc_wg_per_cu = 7;          // k_sc_cf: persistent workgroups per CU
    int sc128_one_wave = 1;        // k_sc_cf over <= 960 lags: one wavefront per frame (two chunks per lane, 15 frames per CU, no wavefront idling through the fine pass) instead of two (0: A/B); measured 1.46 -> 1.31 ms per 262 144 config-3 frames over all lags, 1.43 -> 1.25 bounded
    int sc_first_lags = 576;       // k_sc_cf, searches of >= twice as many lags: the lags the first launch looks at (0 = one launch over every lag).
                                   // 576 = a crossing up to lag 335 with its whole window of W = 240 lags: a packet that starts within ~250 samples of its slot.
                                   // Round 3 used 384 (config 3's delay <= 64); round 4's sweep (round-4 script tools/first_lags_sweep.py, since removed, 262 144 frames, one box): the first
                                   // launch costs the same up to 576 lags (early packets: 0.48 ms at 384, 0.49 at 576, 0.71 from 592 on), while on late
                                   // packets (delay 1..401, 10 % empty slots) every lag more decides more frames: search 1.42 -> 0.93 ms, chain 2.05 -> 1.59 ms
    int demod64_wg_per_cu = 0;     // k_demod64: persistent workgroups per CU (0 = from the occupancy API)
    int demod64_burst = 16;        // k_demod64: groups per store burst (16 / 8 / 4; 1 = no bursts)
    int demod64_narrow_stores = 0; // k_demod64: 4-byte instead of 16-byte image stores
    int demod64_store_policy = 0;  // k_demod64: cache-policy bits on the 16-byte image stores (0 default, 1 nt, 2 sc1, 3 sc0 sc1): the output-buffer populations probe
    int scb_two_segments = 0;      // k_scb_chunks: two-segment staging also for L <= 1280
    int scb_big_tiles = 0;         // k_scb_fine: 1280-lag tiles / 128 threads
    int debug_demod64 = 0, debug_sc = 0, debug_tx = 0; // profile build only (kProfile)
    int chest_solve_only = 0;      // ofdm_chest_smooth_batch: 1 = launch k_chest_solve alone on the rows given (into the workspace; nothing is delivered): its time on its own
    int soft_chunk_frames = 0;     // OFDM_ECC_HAMMING74_SOFT / OFDM_ECC_CONV_K7 decode: frames per k_sym<llr> + k_rx_finish_soft / k_viterbi_k7 step (0 = the LLR workspace's 256 MB bound)
    int fcs_bitserial = 0;         // k_fcs_wrap / k_fcs_check: every lane reduces its chunk bit by bit in registers instead of through the slice-by-4 tables in LDS (A/B)
    int no_demod64_sc16 = 0;       // EXT-9: ofdm_rx_demod_sc16_batch at N = 64 widens into the workspace and runs the fc32 path instead of k_demod64_sc16 (A/B)
    int sc16_chunk_frames = 0;     // EXT-9 / EXT-10: frames per k_sc16_widen + fc32 chain step of the sc16 receive entry points and per fc32 encode + k_sc16_narrow
                                   // step of ofdm_tx_encode_sc16_batch's two-pass path (0 = about 48 MB of fc32 samples)
    int no_txframe64_sc16 = 0;     // EXT-10: ofdm_tx_encode_sc16_batch at N = 64 encodes fc32 frames into the workspace and narrows them instead of k_txframe64_sc16 (A/B)
    int scan_mark_only = 0;        // EXT-12: ofdm_sc_scan_long launches k_sc_mark alone and reports no detection: the kernel's time on its own
    int packets_chunk_rows = 0;    // EXT-13: packets per k_gather_rows + chain step of ofdm_rx_decode_packets (0 = as many as keep the gathered rows within 256 MiB)
    int packets_gather_only = 0;   // EXT-13: ofdm_rx_decode_packets launches k_pkt_rows + k_gather_rows alone and delivers nothing: the kernel's time on its own
    int stream_scan_cap = 0;       // EXT-14: detections per scan + decode round of ofdm_stream_push (0 = 256; the tests force 2, so that the round loop runs)
};
inline const Tuning &tuning_or_default(const Tuning *t) { static const Tuning d; return t ? *t : d; }

// Which kernels served the last entry point (ofdm_last_dispatch): every launcher appends the kernel it really launched, in launch
// order.  Only an entry point's scope resets it (EntryScope, ofdm_ctx.hpp); launches the string leaves out on purpose -- the chunks
// behind the first of a chunk loop -- run under a Mute.
struct Trace {
    char buf[256] = {};
    int len = 0;
    int muted = 0;
    void reset() { len = 0; buf[0] = 0; }
    void add(const char *name) {
        if (muted) return;
        if (len && len < (int)sizeof(buf) - 1) buf[len++] = '+';
        while (*name && len < (int)sizeof(buf) - 1) buf[len++] = *name++;
        buf[len] = 0;
    }
    struct Mute { // add() does nothing while one is alive (on = false: a guard that does nothing, for `Mute later(trace, f0 > 0)`)
        Trace &t;
        const bool on;
        explicit Mute(Trace &t, bool on = true) : t(t), on(on) { t.muted += on; }
        ~Mute() { t.muted -= on; }
        Mute(const Mute &) = delete;
        Mute &operator=(const Mute &) = delete;
    };
};
inline void trace_add(Trace *t, const char *name) { if (t) t->add(name); }

// ---- launcher plumbing shared by the kernels_*.hip files
// Run-time value -> template argument: calls f(std::integral_constant<int, V>{}) for the V of the list that equals v (the callee
// reads it as decltype(V)::value); a value outside the list is hipErrorNotSupported, the launchers' "not this fast path".
template <int... Vs, class F> hipError_t with_int(int v, F &&f) {
    hipError_t e = hipErrorNotSupported;
    (void)((v == Vs && ((e = f(std::integral_constant<int, Vs>{})), true)) || ...);
    return e;
}
template <class F> hipError_t with_bool(bool b, F &&f) { return b ? f(std::true_type{}) : f(std::false_type{}); }
template <class F> hipError_t with_bps(int bps, F &&f) { return with_int<1, 2, 4, 6, 8>(bps, f); } // bits per constellation point
// Persistent grid: one workgroup per unit of work, at most `resident` of them (workgroups per CU x CUs), at most Tuning::grid_cap
inline long long persistent_grid(long long units, long long resident, const Tuning &tu) {
    if (tu.grid_cap > 0 && tu.grid_cap < resident) resident = tu.grid_cap;
    return units < resident ? units : resident;
}

// Persistent grid: resident workgroups per CU from the occupancy API (per instantiation and device, cached), doubled up
// to the 8 the round-1 launcher used -- measured (OFDM_DEMOD64_WG_PER_CU sweep, 1 M frames): 3 -> 1.77 ms, 4 -> 1.70,
// 5 -> 1.81, 8 -> 1.68: a second, queued round of workgroups evens out the tail.
// The cache is keyed by the kernel's ADDRESS: every k_demod64 instantiation has the same function type, so a static inside a
// template over that type would be shared by all of them (the BURST = 16 variant holds 37 KB of LDS per workgroup, the others 11).
template <typename K> inline int resident_blocks(K kernel, int block) {
    struct Entry { const void *fn; int dev, n; };
    static Entry cache[64];
    static int used = 0;
    static std::mutex mtx;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    const void *fn = reinterpret_cast<const void *>(kernel);
    std::lock_guard<std::mutex> lock(mtx);
    for (int i = 0; i < used; ++i) if (cache[i].fn == fn && cache[i].dev == dev) return cache[i].n;
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, block, 0) != hipSuccess || n < 1) n = 4;
    n = n > 8 ? 8 : n;
    if (used < 64) cache[used++] = Entry{fn, dev, n};
    return n;
}

// Counters of the last Schmidl-Cox search on a context (ofdm_get_tuning "stat_sc_slow_frames" / "stat_sc_redo_frames"): how many
// frames went to the all-f64 kernel, and how many the first launch of the two-launch search left to the whole search.  `dev` is a
// small device buffer OWNED BY THE CONTEXT ([0] slow, [1] redo): the search copies its counters there on its stream, so that the
// figures survive the search's workspace being regrown or reused by another entry point.
struct ScStats {
    int32_t *dev = nullptr;
    bool has_slow = false, has_redo = false;
};

struct SymParams {
    const Tuning *tune = nullptr; // nullptr = defaults
    Trace *trace = nullptr;
    // input samples / bins
    const float2 *in = nullptr;
    long long n_frames = 0;
    long long frame_stride = 0; // samples between frame bases
    long long frame_len = 0;    // valid samples per frame; reads at or beyond it return 0 (pad_chunk)
    int syms_per_frame = 1;
    int first_symbol = 0;       // symbol index (in units of in_sym_stride) of symbol 0
    int in_sym_stride = 0;      // samples between consecutive symbols in the input
    int in_skip = 0;            // samples skipped at the start of each symbol (cyclic prefix) on input
    int sym_len = 0;            // S = N + CP
    const int32_t *offset = nullptr;     // per-frame sample offset of the trimmed frame start
    const double *f_delta = nullptr;     // per-frame CFO (rad/sample); sample ids count from offset[f]
    const int32_t *nsym_frame = nullptr; // per-frame number of live symbols (demod)
    // channel / tables
    const float2 *hk = nullptr;
    long long hk_stride = 0;
    const float2 *tw = nullptr;           // exp(-2 pi i m / N)
    const float2 *inv_training = nullptr; // 1 / training[k]
    // outputs
    float2 *out = nullptr;       // FFT / IFFT(+CP) / channel estimate / TX frames
    long long out_stride_s = 0;  // TX: samples between output frames
    unsigned char *out_bytes = nullptr;
    long long out_stride = 0;    // bytes between per-frame outputs
    float2 *soft = nullptr;
    // modulation / TX
    int bps = 1;
    int guard = 0;
    // (k_sym<llrw> reads no payload: there the two words hold the rows of per-bin LLR weights, EXT-11.  The struct keeps its layout,
    // and with it every kernel that takes it keeps its kernel descriptor.)
    union { const uint8_t *payload = nullptr; const float *bin_weight; };
    union { long long payload_stride = 0; long long bin_weight_stride; }; // bin_weight_stride: floats between the frames' rows, 0 = one shared row
    const int32_t *payload_len = nullptr;
    int payload_bytes = 0;
    unsigned *frame_max = nullptr; // per-frame max(0, re, im) as float bits
    long long tx_raw_total = -1;   // >= 0: TX of a continuous symbol stream (modulate + encode_block + prefix_block only):
                                   // payload is tx_raw_total plain bytes, one symbol per "frame", no length header, no frame
                                   // header blocks, no normalise
    // LLR demod (k_sym<llr>): int8 max-log LLRs, syms_per_frame * data_carriers * bps per frame (include/ofdm_hip.h)
    int8_t *llr = nullptr;
    float llr_scale = 0.f;
    long long llr_stride = 0;    // bytes between per-frame LLR rows
};

// N = 64 RX-demod fast path (kernels_n64.hip)
struct Fast64Params {
    const float2 *in = nullptr;
    long long frame_stride = 0;
    int first_symbol = 0;
    const float2 *hk = nullptr; // shared channel or nullptr
    const float2 *tw = nullptr;
    unsigned char *out = nullptr;
    long long out_stride = 0;
    int groups_per_frame = 1;   // 8-symbol groups per frame
    long long n_groups = 0, stride_groups = 0;
    long long f0 = 0, blk_df = 0, wave_df = 0, step_df = 0; // frame index bookkeeping without division
    int k0 = 0, blk_dk = 0, wave_dk = 0, step_dk = 0;
    int wide_stores = 0;        // the packed image leaves with 16-byte stores (aligned output)
    int store_policy = 0;       // lab key demod64_store_policy: cache-policy bits on the image stores (0 default, 1 nt, 2 sc1, 3 sc0 sc1)
    int debug = 0;              // profiling aid (OFDM_DEMOD64_DEBUG): 1 no stores, 2 no packing either, 3 loads + first butterfly only
};
hipError_t run_demod64_fast(const SymParams &p, hipStream_t st, int num_cu);
// EXT-9: the same kernel body fed with sc16 samples (kernels_n64_sc16.hip).  One dword = (int16 re, int16 im), little-endian; every
// component is widened as (float)v * scale, one rounded f32 product (include/ofdm_hip.h).  p.in is not read.
struct Fast64Sc16Params : Fast64Params {
    const uint32_t *in16 = nullptr;
    float scale = 0.f;
};
// run_demod64_fast's envelope with a 4-byte aligned input; hipErrorNotSupported outside it (caller widens and takes the fc32 path)
hipError_t run_demod64_sc16(const SymParams &p, const uint32_t *in16, float scale, hipStream_t st, int num_cu);

// ---- EXT-9 sc16 <-> fc32 (ofdm_sc16_widen_batch / ofdm_sc16_narrow_batch and the widen step of the sc16 receive entry points;
// kernels_sc16.hip, definition: include/ofdm_hip.h, tests/sc16_ref.py).  Rows of frame_len samples, strides in samples.
struct Sc16Params {
    const Tuning *tune = nullptr;
    Trace *trace = nullptr;
    long long n_frames = 0, frame_len = 0, in_stride = 0, out_stride = 0;
    float scale = 0.f;
    const uint32_t *sc_in = nullptr;     // widen: sc16 in, fc32 out
    float2 *fc_out = nullptr;
    const float2 *fc_in = nullptr;       // narrow: fc32 in, sc16 out
    uint32_t *sc_out = nullptr;
    int32_t *clipped = nullptr;          // narrow, optional: clipped components per row
};
hipError_t run_sc16_widen(const Sc16Params &p, int num_cu, hipStream_t st);
hipError_t run_sc16_narrow(const Sc16Params &p, int num_cu, hipStream_t st);
// the two host functions behind ofdm_sc16_widen / ofdm_sc16_narrow (scale already checked)
void sc16_widen_host(const int16_t *in, long long n, float scale, float *out);
long long sc16_narrow_host(const float *in, long long n, float scale, int16_t *out);
// N = 4096 RX demod as 64 x 64 (regular streams: no offset / CFO / per-frame symbol counts / soft output)
hipError_t run_demod4096(const SymParams &p, hipStream_t st, int num_cu);
// fused estimate_channel + per-symbol demod [+ finish] for N = 1024 frames (16 x 64 FFT, kernels_rx1024.hip), the N = 1024
// analogue of run_rxframe64.  final_* (optional): length header, truncate and Hamming decode done by the same kernel when the
// frame's packed bytes fit its LDS image; *fused_out reports whether they were (else the caller runs k_rx_finish).  A frame that
// must not be decoded is one with nsym_frame[f] == 0 (the prepare kernels guarantee it for every status != 0).
hipError_t run_rxframe1024(const SymParams &p, float2 *hk_out, hipStream_t st, int num_cu, unsigned char *final_out = nullptr,
                           long long final_stride = 0, int32_t *final_len = nullptr, int ecc = 0, bool *fused_out = nullptr);
// N = 4096 continuous-stream TX (map + IFFT + CP) as 64 x 64; needs tx_raw_total >= 0
hipError_t run_tx4096(const SymParams &p, hipStream_t st, int num_cu);
hipError_t run_txframe4096(const SymParams &p, const float2 *header, float header_max, hipStream_t st, int num_cu);
// N = 128 .. 2048 symbol-stream fast paths (kernels_mid.hip); hipErrorNotSupported => generic k_sym
hipError_t run_demod_mid(int n_fft, const SymParams &p, hipStream_t st, int num_cu);
hipError_t run_tx_mid(int n_fft, const SymParams &p, hipStream_t st, int num_cu);
hipError_t run_txframe_mid(int n_fft, const SymParams &p, const float2 *header, float header_max, hipStream_t st, int num_cu);
// fused estimate_channel + per-symbol demod for N = 64 frames with per-frame offset / CFO / live-symbol count
// final_out / final_stride / final_len (optional, 4-byte aligned): also do the length-header parse + truncate and write the
// payload bytes to their final place (no outer code), so that no separate finish kernel is needed
// frame_list / frame_count (device, optional): only the listed frames are processed
// cut_ws (device, optional, n_frames + 4 ints): the split form -- one launch with only the common frame body (four waves per SIMD) over
// every frame, one with only the capture-cut body over the frames the first one left on the list in cut_ws
hipError_t run_rxframe64(const SymParams &p, float2 *hk_out, hipStream_t st, int num_cu, unsigned char *final_out = nullptr,
                         long long final_stride = 0, int32_t *final_len = nullptr, const int32_t *frame_list = nullptr,
                         const int32_t *frame_count = nullptr, int32_t *cut_ws = nullptr);
// fused encode for N = 64 (map + IFFT + CP + header + normalise, one HBM pass); hipErrorNotSupported outside its envelope
hipError_t run_txframe64(const SymParams &p, const float2 *header, float header_max, hipStream_t st, int num_cu);
// EXT-10: the same frame loop storing sc16 samples (kernels_n64_tx_sc16.hip): row f = ofdm_sc16_narrow(frame f of run_txframe64, scale),
// clipped (optional) = its count per frame.  p.out / p.out_stride_s are not read.  run_txframe64's envelope with out16 16-byte aligned
// and out_stride (samples) a multiple of 4 -- txframe64_sc16_takes, which the caller asks before it codes the rows; outside it the
// caller encodes fc32 frames and runs k_sc16_narrow
bool txframe64_sc16_takes(int n_sym, const void *out16, long long out_stride);
hipError_t run_txframe64_sc16(const SymParams &p, const float2 *header, float header_max, uint32_t *out16, long long out_stride, float scale,
                              int32_t *clipped, hipStream_t st, int num_cu);

hipError_t run_fft(int n, const SymParams &p, bool inverse, hipStream_t st, int num_cu);
hipError_t run_ifft_cp(int n, const SymParams &p, hipStream_t st, int num_cu);
hipError_t run_demod(int n, const SymParams &p, hipStream_t st, int num_cu);
hipError_t run_chest(int n, const SymParams &p, hipStream_t st, int num_cu);
hipError_t run_tx_symbols(int n, const SymParams &p, hipStream_t st, int num_cu);
// LLR demod: the RX demod chain with int8 max-log LLRs out (p.llr) and, when p.out_bytes is set, the hard bytes too
hipError_t run_llr(int n, const SymParams &p, hipStream_t st, int num_cu);
// EXT-11: run_llr with the LLR scale of bin k multiplied by p.bin_weight[f * p.bin_weight_stride + k] (k_sym<llrw>)
hipError_t run_llrw(int n, const SymParams &p, hipStream_t st, int num_cu);

// ---- EXT-6 link quality (ofdm_rx_quality_batch; kernels_quality.hip, definition: tests/quality_ref.py)
// k_linkq: one row of kQualityFields floats per frame from the five training blocks (noise variance, gain, SNR, LLR unit) and the
// decision-directed EVM of the frame's first n_points[f] data points.  A frame with status[f] != 0 is not read and gets a zero row.
constexpr int kQualityFields = 8;
struct LinkqParams {
    const Tuning *tune = nullptr;
    Trace *trace = nullptr;
    const float2 *in = nullptr;
    long long n_frames = 0, frame_stride = 0, frame_len = 0;
    int first_symbol = 0, syms_per_frame = 0;
    int sym_len = 0;                     // S = N + CP
    const int32_t *n_points = nullptr;   // optional: occupied constellation points per frame (nullptr: no EVM)
    const int32_t *offset = nullptr;
    const double *f_delta = nullptr;
    const int32_t *status = nullptr;     // optional
    const float2 *hk = nullptr;
    long long hk_stride = 0;
    const float2 *tw = nullptr;
    int bps = 1, guard = 0;
    float inv_t2 = 0.f;                  // 1 / sum over the data carriers of |t_k|^2
    float es = 1.f;                      // mean |point|^2 of the constellation
    float *quality = nullptr;            // [n_frames][kQualityFields]
};
hipError_t run_linkq(int n, const LinkqParams &p, hipStream_t st, int num_cu);
// the two constants of a context: training = n interleaved (re, im) doubles; bps = bits per constellation point
float linkq_inv_t2(const double *training, int n, int guard);
float linkq_es(int bps);

// ---- EXT-7 soft combining (ofdm_llr_combine_batch and the combine step of ofdm_rx_decode_combine_batch; kernels_combine.hip,
// definition: tests/combine_ref.py)
// k_llr_combine: branch r of frame f is row f * n_branches + r of llr, quality, status, n_live and weight; one combined row a frame.
constexpr int kCombineMaxBranches = 8;
struct CombineParams {
    const Tuning *tune = nullptr;
    Trace *trace = nullptr;
    const int8_t *llr = nullptr;
    long long n_frames = 0, llr_stride = 0;
    int n_branches = 1;
    int n_llr = 0;
    const float *quality = nullptr;      // optional rows of kQualityFields floats (nullptr: every branch with status 0 is live, u = 1)
    const int32_t *status = nullptr;     // optional
    const int32_t *n_live = nullptr;     // optional: branch row counts for j < clamp(n_live * live_unit, 0, n_llr)
    int live_unit = 1;                   // stage: 1; chain: n_live holds live SYMBOLS, live_unit = data_carriers * bps
    int8_t *out = nullptr;
    long long out_stride = 0;
    int32_t *weight = nullptr;           // optional: q_r per branch row
    // chain only (both or neither): the merged status and the largest n_live entry over the live branches, per frame
    int32_t *status_out = nullptr, *nsym_out = nullptr;
};
hipError_t run_llr_combine(const CombineParams &p, int num_cu, hipStream_t st);

// ---- EXT-8 wide CFO acquisition (ofdm_cfo_wide_batch and the OFDM_CFO_WIDE receive mode; kernels_cfowide.hip, definition:
// tests/cfo_wide_ref.py)
// k_cfo_wide: per frame the hypothesis m in [-span, span] whose training blocks, derotated by f_delta[f] + 2 pi m / S and matched against
// the training table, put the most energy into the channel window; f_delta[f] becomes that sum (untouched for m = 0 and for a frame
// that is not tested: status[f] != 0, or the five training blocks not wholly inside the capture).
constexpr int kCfoWideMaxSpan = 32;
struct CfoWideParams {
    const Tuning *tune = nullptr;
    Trace *trace = nullptr;
    const float2 *in = nullptr;
    long long n_frames = 0, frame_stride = 0, frame_len = 0;
    int sym_len = 0;                     // S = N + CP
    int span = 0;                        // 1 .. kCfoWideMaxSpan
    const int32_t *offset = nullptr;
    const int32_t *status = nullptr;     // optional
    double *f_delta = nullptr;           // in: f0, out: f0 + 2 pi m / S
    const float2 *tw = nullptr;
    const float2 *trn = nullptr;         // the training table t_k
    int32_t *m = nullptr;                // optional
    float *metric = nullptr;             // optional: [n_frames][2] = G of m, the largest G among the other hypotheses
};
hipError_t run_cfo_wide(int n, const CfoWideParams &p, hipStream_t st, int num_cu);

// ---- EXT-11 noise-aware LLR weights (ofdm_rx_noise_bins_batch and the OFDM_LLRW_NOISE receive mode; kernels_noise.hip, definition:
// tests/noise_weight_ref.py)
// k_noise_bins: per frame the noise variance of every received bin from the scatter of the five training blocks, s_k = (1/4) sum_b
// |FFT(y_b - ybar)[k]|^2, and the weight q_k = mean(s) / s_k where s_k > mean(s), else 1.  A frame that is not tested (status[f] != 0, or
// the five training blocks not wholly inside the capture) is not read and gets s = 0, q = 1.
struct NoiseBinsParams {
    const Tuning *tune = nullptr;
    Trace *trace = nullptr;
    const float2 *in = nullptr;
    long long n_frames = 0, frame_stride = 0, frame_len = 0;
    int sym_len = 0;                     // S = N + CP
    const int32_t *offset = nullptr;
    const double *f_delta = nullptr;     // optional
    const int32_t *status = nullptr;     // optional
    const float2 *tw = nullptr;
    float *nvar = nullptr;               // optional: [n_frames][N] = s_k
    float *weight = nullptr;             // optional: [n_frames][N] = q_k
};
hipError_t run_noise_bins(int n, const NoiseBinsParams &p, hipStream_t st, int num_cu);

// ---- Schmidl-Cox (kernels_sync.hip)
struct ScParams {
    const Tuning *tune = nullptr;
    Trace *trace = nullptr;
    const float2 *in = nullptr;
    long long n_frames = 0, frame_stride = 0, frame_len = 0;
    long long n_lags = 0;        // lags searched per frame (already clipped to the valid range)
    int L = 0, W = 0;            // period and window
    double threshold = 0.5;
    bool tail_mapped = false;    // the sample behind every frame's last one is mapped memory (rows with slack, or not the batch's last row)
    int tiles_per_frame = 1;
    int mode = 0;                // 0 fused (single tile), 1 first-crossing only, 2 peak search from lag_base
    const int32_t *lag_base = nullptr; // mode 2: per-frame first lag (d1), -1 = skip
    long long *cross = nullptr;        // mode 1: per-tile first crossing (or LLONG_MAX)
    int32_t *d_hat = nullptr;
    double *f_delta = nullptr;
    float *metric = nullptr;
    const int32_t *slow_list = nullptr;  // k_sc_tile list mode: frames to (re)do, count in *slow_count
    const int32_t *slow_count = nullptr;
    ScStats *stats = nullptr;            // optional: where the search leaves the addresses of its list counters
};
struct ScExact { double pr, pi, num, den; }; // exact sums at the chosen lag; k_sc_post turns them into CFO and metric
size_t sc_lds_bytes(const ScParams &p);
// L = 80, W = 240 (N = 64): every lag on f64 prefix differences, one streaming pass that stops when the peak window has closed
// (kernels_sc80.hip).  Leaves d_hat and the exact sums of the chosen lag (k_sc_post's input); frames it does not trust go to slow_list.
bool sc80_ok(const ScParams &p);
bool sc80_wanted(const ScParams &p);   // sc80_ok and enough frames (or short enough slots) for one row per frame to pay
hipError_t launch_sc80(const ScParams &p, ScExact *exact, int32_t *slow_list, int32_t *slow_count, int num_cu, hipStream_t st);
hipError_t run_sc(const ScParams &p, hipStream_t st);
// fast path for one-tile frames with a short period (f32 filter + exact f64 decisions; kernels_sync.hip)
bool sc_fast_ok(const ScParams &p);
size_t sc_fast_workspace_bytes(long long n_frames, long long n_lags);
hipError_t run_sc_fast(const ScParams &p, void *workspace, int num_cu, hipStream_t st);
// periods L = 160 .. 1280 (N = 128 .. 1024): one streaming pass per frame that stops once the decision is determined
// (kernels_scstream.hip)
bool sc_stream_ok(const ScParams &p);
hipError_t run_sc_stream(const ScParams &p, int num_cu, hipStream_t st);
// long periods (N >= 128): chunk sums + bounded exact search (kernels_scbig.hip)
struct ScBigParams {
    const float2 *in = nullptr;
    long long n_frames = 0, frame_stride = 0, frame_len = 0, n_lags = 0;
    int L = 0, W = 0, C = 0;       // period, window, chunk = L / 8
    int nch = 0, nch_pad = 0;      // chunks per frame; row length of the workspace (>= nch + 1)
    int tiles_per_frame = 0;
    double threshold = 0.5;
    double *ws = nullptr;          // [n_frames][3][nch_pad]: chunk totals, then exclusive prefixes, of q.re, q.im, e
    int32_t *d_hat = nullptr;
    double *f_delta = nullptr;
    float *metric = nullptr;
};
bool sc_big_ok(const ScParams &p);
size_t sc_big_workspace_bytes(const ScParams &p);
hipError_t run_sc_big(const ScParams &p, void *workspace, int num_cu, hipStream_t st);
hipError_t run_sc_min_cross(const long long *cross, int tiles_per_frame, long long n_frames, int32_t *d1, hipStream_t st);
// ---- EXT-12 every detection of one long capture (ofdm_sc_scan_long; kernels_scscan.hip, definition: tests/scan_ref.py)
// k_sc_mark: bit j of `bits` = lag lag_lo + j crosses the threshold (den > 0 && num >= threshold den), j < n_lags; k_sc_walk: d1[0] =
// the first crossing, d1[k + 1] = the first crossing at or after d1[k] + holdoff, at most det_cap of them, head = {n_det, more}; k_sc_peaks:
// row k of d_hat / f_delta / metric = the first maximum of the metric over [d1[k], min(d1[k] + W, valid - 1)].
// The caller guarantees 0 <= lag_lo, n_lags >= 1 and lag_lo + n_lags <= valid = n_samples - W - L + 1.
struct ScScanParams {
    const Tuning *tune = nullptr;
    Trace *trace = nullptr;
    const float2 *in = nullptr;
    long long valid = 0, lag_lo = 0, n_lags = 0, holdoff = 1, det_cap = 0;
    int L = 0, W = 0;
    double threshold = 0.5;
    unsigned long long *bits = nullptr;  // ceil(n_lags / 64) words
    long long *head = nullptr;           // [2]
    long long *d1 = nullptr, *d_hat = nullptr; // [det_cap]
    double *f_delta = nullptr;
    float *metric = nullptr;
};
hipError_t run_sc_mark(const ScScanParams &p, int num_cu, hipStream_t st);  // k_sc_mark alone
hipError_t run_sc_scan(const ScScanParams &p, int num_cu, hipStream_t st);  // k_sc_mark + k_sc_walk + k_sc_peaks
// ---- EXT-13 every packet of one long capture as rows of one batch (ofdm_rx_decode_packets; kernels_packets.hip, definition:
// tests/packets_ref.py).  k_pkt_rows: per packet k < n_det the row start r_k = max(d_hat[k] - L - backoff, 0) & ~1, row_dhat = d_hat[k] -
// r_k, row_len = min(R, n - r_k), f_delta[k] = f_delta_in[k], metric[k] = metric_in[k] (metric optional).  k_gather_rows: rows[j] =
// capture[r : r + R] for r = row_start[row0 + j], j < n_rows, zeros at and beyond sample n; R even, rows 16-byte aligned, in 8-byte aligned.
struct PktParams {
    const Tuning *tune = nullptr;
    Trace *trace = nullptr;
    const float2 *in = nullptr;
    long long n = 0, n_det = 0, R = 0, row0 = 0, n_rows = 0;
    int L = 0, backoff = 0;
    const long long *d_hat = nullptr;    // [n_det] on the device, each in [0, n)
    const double *f_delta_in = nullptr;
    const float *metric_in = nullptr;
    long long *row_start = nullptr;      // [n_det]
    int32_t *row_dhat = nullptr, *row_len = nullptr;
    double *f_delta = nullptr;
    float *metric = nullptr;
    float2 *rows = nullptr;              // [n_rows][R]
};
hipError_t run_pkt_rows(const PktParams &p, hipStream_t st);
hipError_t run_gather_rows(const PktParams &p, int num_cu, hipStream_t st);
// k_rx_prepare with a frame_len per row (row_len[f]): status / offset / live symbols / CFO of row f from its own length
hipError_t run_rx_prepare_rows(long long n_rows, const int32_t *d_hat, double *f_delta, const int32_t *row_len, int L, int backoff,
                               int cfo_mode, int max_symbols, int bytes_per_symbol, int32_t *status, int32_t *offset, int32_t *nsym,
                               hipStream_t st);
// offset[k] = row_start[k] + row_offset[k] (0 + row_offset[k] where status[k] is OFDM_FRAME_BADTIMING)
hipError_t run_pkt_finish(long long n_det, const long long *row_start, const int32_t *row_offset, const int32_t *status, long long *offset,
                          hipStream_t st);
// ---- EXT-14 the window of a streaming receiver (ofdm_stream_push; kernels_stream.hip, definition: tests/stream_ref.py).
// k_stream_ingest<fc32> / <sc16>, one launch: win[i] = carry[i] for i < keep, win[keep + j] = chunk[j] (sc16: widened by `scale` as
// k_sc16_widen widens) for j < n; nothing behind win[keep + n) is written.  carry, win and chunk are 16-byte aligned and do not overlap.
struct StreamIngestParams {
    const Tuning *tune = nullptr;
    Trace *trace = nullptr;
    const float2 *carry = nullptr;       // the old window from its first kept sample on
    long long keep = 0, n = 0;
    const void *chunk = nullptr;         // n samples: float2 (fc32) or int16 pairs (sc16)
    float scale = 0.f;                   // sc16 only
    float2 *win = nullptr;               // the new window
};
hipError_t run_stream_ingest(const StreamIngestParams &p, bool sc16, int num_cu, hipStream_t st);
// ---- EXT-15 the DC blocker (ofdm_dcblock_push, ofdm_stream_set_dc_block; kernels_dcblock.hip, definition: tests/dcblock_ref.py).
// k_dc_block<fc32> / <sc16>, one launch: out[e] = x[e] - the f32 mean of the up to `blocks` complete 64-sample blocks in front of the
// block of stream sample t0 + e (block 0: out = x), for e < n, and the state behind the piece into ring_new / open_new.  in and out do
// not overlap; the four state buffers are distinct.
constexpr int kDcMaxBlocks = 1024;
struct DcBlockParams {
    const Tuning *tune = nullptr;
    Trace *trace = nullptr;
    const void *in = nullptr;            // n samples: float2 (fc32) or int16 pairs (sc16)
    float2 *out = nullptr;
    long long n = 0, t0 = 0;             // t0: the samples of the filter's stream in front of the piece
    float scale = 0.f;                   // sc16 only
    int blocks = 0;                      // M, 1 .. kDcMaxBlocks
    const double2 *ring_old = nullptr;   // [M] the sum of block k in slot k % M, for the last M complete blocks in front of the piece
    double2 *ring_new = nullptr;         // ... behind the piece; written only when the piece completes a block
    const float2 *open_old = nullptr;    // [64] the t0 % 64 samples of the open block in front of the piece
    float2 *open_new = nullptr;          // ... the (t0 + n) % 64 behind it; written whenever that is not 0
};
hipError_t run_dc_block(const DcBlockParams &p, bool sc16, int num_cu, hipStream_t st);
// ---- EXT-16 the down-converter (ofdm_ddc_push, ofdm_stream_set_ddc; kernels_ddc.hip, definition: tests/ddc_ref.py).
// k_ddc<fc32> / <sc16>, one launch: out[m - M(t0)] = y[m] for M(t0) <= m < M(t0 + n) (M: ddc_out_len), and the raw samples behind the
// piece's last output into carry_new.  in and out do not overlap; the two carries are distinct.
constexpr int kDdcMaxDecim = 64, kDdcMaxTaps = 4096;
constexpr long long kDdcPhaseMask = (1 << 20) - 1;
inline long long ddc_out_len(long long n, int decim, int n_taps) { return n < n_taps ? 0 : (n - n_taps) / decim + 1; }
struct DdcParams {
    const Tuning *tune = nullptr;
    Trace *trace = nullptr;
    const void *in = nullptr;            // n samples: float2 (fc32, on 8 bytes) or int16 pairs (sc16, on 4 bytes)
    float2 *out = nullptr;               // M(t0 + n) - M(t0) samples
    long long n = 0, t0 = 0;             // t0: the samples of the converter's stream in front of the piece
    float scale = 0.f;                   // sc16 only
    int decim = 0, n_taps = 0;           // D, T
    unsigned phase_inc = 0;              // mod 2^20
    const float *taps = nullptr;         // [T]
    const float2 *coarse = nullptr, *fine = nullptr; // [1024] each: the rotor tables
    const float2 *carry_old = nullptr;   // the raw (widened) samples D M(t0) .. t0 - 1 of the stream
    float2 *carry_new = nullptr;         // ... D M(t0 + n) .. t0 + n - 1; at most T - 1 of them
};
hipError_t run_ddc(const DdcParams &p, bool sc16, int num_cu, hipStream_t st);
// base (optional): per-pair sample offset added to the pair's start; status (optional): pairs with status != 0 get 0
hipError_t run_freq_correction(const float2 *in, long long n_pairs, long long stride, long long right_offset, int L,
                               double *f_delta, hipStream_t st, const int32_t *base = nullptr, const int32_t *status = nullptr);
// xcorr_fft (src/signals/mod.rs:186-217) of every capture a[f] (N samples) with b (nb samples): idx_max into the fft_shifted
// 2N - 1 output, |.| at it, optionally the whole output
size_t xcorr_workspace_bytes(long long n_frames, long long N, int nb);
hipError_t run_xcorr(const float2 *a, long long n_frames, long long stride, long long N, const float2 *b, int nb, void *workspace,
                     int32_t *idx_max, float *peak, float2 *out, long long out_stride, int num_cu, hipStream_t st);
// reference timing -> trimmed offset (src/receiver.rs:21-36): offset = idx_max - N.  offset_report (optional) receives that
// value as it is (negative for quirk Q1), offset_kernels the copy the receive kernels index with (0 unless status == 0)
hipError_t run_rx_prepare_ref(long long n_frames, const int32_t *idx_max, long long frame_len, int L, int max_symbols,
                              int bytes_per_symbol, int32_t *status, int32_t *offset_report, int32_t *offset_kernels, int32_t *nsym,
                              hipStream_t st);
hipError_t run_cfo_rotate(float2 *x, long long n_frames, long long frame_stride, long long frame_len,
                          const double *f_delta, const int32_t *first_index, hipStream_t st);

// ---- byte / elementwise kernels (kernels_bytes.hip)
hipError_t run_qam_map(const uint8_t *bytes, long long n_bytes, int bps, float2 *out, hipStream_t st);
hipError_t run_qam_demap(const float2 *sym, long long n_sym, int bps, uint8_t *bytes, uint8_t *idx, hipStream_t st);
hipError_t run_encode_block(const float2 *data, float2 *bins, long long n_sym, int n_fft, int guard, hipStream_t st);
hipError_t run_frame_max(const float2 *x, long long n_frames, long long frame_stride, long long frame_len,
                         unsigned *frame_max, hipStream_t st);
hipError_t run_frame_scale(float2 *x, long long n_frames, long long frame_stride, long long frame_len,
                           const unsigned *frame_max, hipStream_t st);
hipError_t run_ham_encode(const uint8_t *in, long long n_frames, long long in_stride, const int32_t *in_len,
                          long long n_bytes, uint8_t *out, long long out_stride, int32_t *out_len, hipStream_t st);
hipError_t run_ham_decode(const uint8_t *in, long long n_bytes, uint8_t *out, uint32_t *corrected, hipStream_t st);
// TX finish: write the 10 header blocks and divide the frame by its max (transmitter.rs:183-194)
hipError_t run_tx_finish(float2 *out, long long n_frames, long long out_stride, int header_len, long long frame_len,
                         const float2 *header, float header_max, const unsigned *frame_max, hipStream_t st);
// RX prepare: d_hat -> status / offset / live symbols / CFO (receiver.rs:21-39)
hipError_t run_rx_prepare(long long n_frames, const int32_t *d_hat, double *f_delta, long long frame_len, int L,
                          int backoff, int cfo_mode, int max_symbols, int bytes_per_symbol, int32_t *status,
                          int32_t *offset, int32_t *nsym, hipStream_t st, const int32_t *frame_list = nullptr,
                          const int32_t *frame_count = nullptr);
// one capture's timing written where the search would have left it (DecodeCall::known: ofdm_rx_decode_long with lag_lo > 0)
hipError_t run_set_sync(int32_t *d_hat, double *f_delta, float *metric, int32_t d, double fd, float m, hipStream_t st);
// RX finish: header parse + truncate [+ Hamming decode] (receiver.rs:85-95)
hipError_t run_rx_finish(const uint8_t *raw, long long raw_stride, long long n_frames, const int32_t *status,
                         const int32_t *nsym, int bytes_per_symbol, int ecc, uint8_t *out, long long out_stride,
                         int32_t *out_len, hipStream_t st, const int32_t *frame_list = nullptr,
                         const int32_t *frame_count = nullptr);
// soft RX finish (OFDM_ECC_HAMMING74_SOFT): the header from the hard bytes as k_rx_finish, the body ML-decoded from the LLR rows
// (llr row f holds the frame's LLRs from stream bit 0; the body starts at LLR 128)
hipError_t run_rx_finish_soft(const uint8_t *raw, long long raw_stride, const int8_t *llr, long long llr_stride, long long n_frames,
                              const int32_t *status, const int32_t *nsym, int bytes_per_symbol, uint8_t *out, long long out_stride,
                              int32_t *out_len, hipStream_t st);
// soft Hamming(7,4) decode of n_bits / 56 blocks of 8 codewords (ofdm_hamming74_decode_soft)
hipError_t run_ham_decode_soft(const int8_t *llr, long long n_bits, uint8_t *out, hipStream_t st);

// ---- K = 7 rate-1/2 convolutional code (OFDM_ECC_CONV_K7; kernels_conv.hip)
// rows of n_bytes payload bytes (row f: in_len[f] of them when in_len is given) -> rows of 2 (n_bytes + 1) coded bytes; out_len
// (optional) receives every row's own coded length 2 (len + 1)
hipError_t run_conv_encode(const uint8_t *in, long long n_frames, long long in_stride, const int32_t *in_len, long long n_bytes,
                           uint8_t *out, long long out_stride, int32_t *out_len, hipStream_t st);
struct ViterbiParams {
    const int8_t *llr = nullptr;   // row f at llr + f * llr_stride
    long long llr_stride = 0, n_frames = 0;
    uint8_t *out = nullptr;
    long long out_stride = 0;
    unsigned long long *surv = nullptr; // survivor workspace: slab_words 8-byte decision words per wavefront of the grid
    long long slab_words = 0;
    // stage mode (raw == nullptr): n_steps steps from LLR 0 of every row, n_steps / 8 bytes out
    int n_steps = 0, terminated = 1;
    // chain mode: steps, termination and out_len from the length header in the frame's hard bytes; the body starts at LLR 128
    const uint8_t *raw = nullptr;
    long long raw_stride = 0;
    const int32_t *status = nullptr, *nsym = nullptr;
    int bytes_per_symbol = 0;
    int32_t *out_len = nullptr;
};
// grid (workgroups of four wavefronts) and slab size for frames of at most max_steps steps; the workspace is blocks * 4 * slab_words * 8 bytes
void viterbi_k7_plan(long long n_frames, long long max_steps, int num_cu, const Tuning *tune, long long *blocks, long long *slab_words);
hipError_t run_viterbi_k7(const ViterbiParams &p, long long blocks, hipStream_t st);

// ---- punctured rates and the framed modes (OFDM_ECC_CONV_K7F_*; kernels_conv.hip, tests/framed_ref.py)
// rate: 0 = 1/2 (nothing dropped), 1 = 2/3 (keep mask (1,1),(1,0) over the steps), 2 = 3/4 ((1,1),(1,0),(0,1)): the 802.11a patterns
constexpr int kConvRates = 3;
constexpr int kConvLengthBlock = 18;     // the framed modes' length block: [u32 LE p][u32 LE ~p] + tail byte at rate 1/2 = 72 steps
// coded bits kept of steps 0 .. T - 1
__host__ __device__ inline long long conv_kept_bits(long long T, int rate) {
    if (rate == 1) return 3 * (T >> 1) + 2 * (T & 1);
    if (rate == 2) { const long long g = T / 3, r = T - 3 * g; return 4 * g + (r == 0 ? 0 : r + 1); }
    return 2 * T;
}
// the largest T with conv_kept_bits(T, rate) <= bits
__host__ __device__ inline long long conv_max_steps(long long bits, int rate) {
    if (rate == 1) { const long long g = bits / 3, r = bits - 3 * g; return 2 * g + (r == 2 ? 1 : 0); }
    if (rate == 2) { const long long g = bits >> 2, r = bits & 3; return 3 * g + (r == 3 ? 2 : r == 2 ? 1 : 0); }
    return bits >> 1;
}
// bytes of the punctured code of p payload bytes and the tail byte, zero-padded to a whole byte
__host__ __device__ inline long long conv_body_len(long long p, int rate) { return (conv_kept_bits(8 * (p + 1), rate) + 7) >> 3; }
// k_conv_encode_p: rows of head + conv_body_len(n_bytes, rate) bytes; head = kConvLengthBlock puts the row's length block in front
// (the framed stream), head = 0 is the bare punctured code.  out_len (optional): every row's own length.
hipError_t run_conv_encode_p(const uint8_t *in, long long n_frames, long long in_stride, const int32_t *in_len, long long n_bytes, int rate,
                             int head, uint8_t *out, long long out_stride, int32_t *out_len, hipStream_t st);
// k_viterbi_k7f.  Stage mode: rows of conv_kept_bits(n_steps, rate) LLRs.  Chain mode: the legacy header is not read; the length block
// is decoded from LLR 128 on, the body from LLR 128 + 144 on, and status becomes OFDM_FRAME_HEADER where there is no valid length.
struct ViterbiFParams : ViterbiParams {
    int rate = 0;
    int32_t *status_rw = nullptr;  // chain mode: read and written (`status` stays unused)
};
hipError_t run_viterbi_k7f(const ViterbiFParams &p, long long blocks, hipStream_t st);

// ---- outer Reed-Solomon(255,223) (ofdm_rs255_*_batch and the OFDM_ECC_RS255* modes; kernels_rs.hip, definition: outer_code.hip)
// rows of n_bytes data bytes (row f: in_len[f], clamped, when in_len is given) -> rows of 255 (n_bytes / 223 + 1) code bytes, zero
// behind the row's own 255 (len_f / 223 + 1); out_len (optional) receives that length
struct Rs255EncodeParams {
    const uint8_t *in = nullptr;
    long long n_frames = 0, in_stride = 0, n_bytes = 0;
    const int32_t *in_len = nullptr;
    uint8_t *out = nullptr;
    long long out_stride = 0;
    int32_t *out_len = nullptr;
};
hipError_t run_rs255_encode(const Rs255EncodeParams &p, int num_cu, const Tuning *tune, hipStream_t st);
// rows of n_code code bytes (row f: code_len[f], clamped, when code_len is given) -> 223 (len_f / 255 + 1) bytes a row; corrected
// (optional): corrected bytes of the row, -1 if a block could not be decoded (its data bytes leave as received).  Chain mode
// (status_rw != nullptr; out_len required, it may be code_len itself): rows with status != 0 are skipped with out_len 0, a row with an
// undecodable block gets status OFDM_FRAME_UNCORRECTABLE and out_len 0.
struct Rs255DecodeParams {
    const uint8_t *code = nullptr;
    long long n_frames = 0, code_stride = 0, n_code = 0;
    const int32_t *code_len = nullptr;
    uint8_t *out = nullptr;
    long long out_stride = 0;
    int32_t *out_len = nullptr, *corrected = nullptr, *status_rw = nullptr;
};
hipError_t run_rs255_decode(const Rs255DecodeParams &p, int num_cu, const Tuning *tune, hipStream_t st);

// ---- CRC-32 frame check (OFDM_ECC_FCS + mode, ofdm_fcs_wrap_batch / ofdm_fcs_check_batch; kernels_fcs.hip, definition: tests/fcs_ref.py)
// IEEE 802.3 CRC-32 of n bytes on the host (ofdm_crc32)
uint32_t crc32_host(const uint8_t *data, long long n);
// k_fcs_wrap: rows of n_bytes payload bytes (row f: in_len[f], clamped, when in_len is given) -> envelopes [u32 LE len][payload][u32 LE
// crc32 of both], zeros behind them up to n_bytes + 8; out_len (optional): every row's len + 8.  chunk and K are the launcher's.
struct FcsWrapParams {
    const uint8_t *in = nullptr;
    long long n_frames = 0, in_stride = 0, n_bytes = 0;
    const int32_t *in_len = nullptr;
    uint8_t *out = nullptr;
    long long out_stride = 0;
    int32_t *out_len = nullptr;
    int chunk = 4;
    unsigned K[6] = {};
};
hipError_t run_fcs_wrap(FcsWrapParams p, int num_cu, const Tuning *tune, hipStream_t st);
// k_fcs_check: rows of n_row bytes (row f: row_len[f], clamped, when row_len is given) -> the payload of a valid envelope at the start
// of the output row (out_stride >= n_row - 8), out_len = its length, ok = 1; out_len = 0, ok = 0 for an invalid row (both optional in
// stage mode).  Chain mode (status_rw != nullptr; out_len required, it may be row_len itself): rows with status != 0 are skipped with
// out_len 0, an invalid row gets status OFDM_FRAME_FCS.
struct FcsCheckParams {
    const uint8_t *row = nullptr;
    long long n_frames = 0, row_stride = 0, n_row = 0;
    const int32_t *row_len = nullptr;
    uint8_t *out = nullptr;
    long long out_stride = 0;
    int32_t *out_len = nullptr, *ok = nullptr, *status_rw = nullptr;
    int chunk = 4;
    unsigned K[6] = {};
};
hipError_t run_fcs_check(FcsCheckParams p, int num_cu, const Tuning *tune, hipStream_t st);

// ---- LDPC(648) (OFDM_ECC_LDPC648 / _R23 / _R34 / _R56, ofdm_ldpc648_encode_batch / _decode_batch and their _rate_batch forms;
// kernels_ldpc.hip, definition: tests/ldpc_ref.py, tests/ldpc_rates_ref.py, ldpc_code.hip).  rate 0 .. 3 = 1/2, 2/3, 3/4, 5/6 with
// K = 40 / 53 / 60 / 67 info bytes a code word, kernels k_ldpc_encode / k_ldpc_decode and k_ldpc_encode<r23|r34|r56> /
// k_ldpc_decode<r23|r34|r56>; any other rate: hipErrorInvalidValue.
// k_ldpc_encode.  Stage mode (framed == 0): rows of n_cw blocks of K info bytes -> n_cw blocks of 80 code bytes.  Chain mode: rows of
// n_bytes payload bytes (row f: in_len[f], clamped, when in_len is given) -> the code of [u32 LE len][u32 LE ~len] ++ payload, zeros
// behind the row's own code words up to n_cw = ceil((n_bytes + 8) / K); out_len (optional): 80 times the row's own count.
struct LdpcEncodeParams {
    const uint8_t *in = nullptr;
    long long n_frames = 0, in_stride = 0, n_bytes = 0, n_cw = 0;
    const int32_t *in_len = nullptr;
    int framed = 0;
    uint8_t *out = nullptr;
    long long out_stride = 0;
    int32_t *out_len = nullptr;
};
hipError_t run_ldpc_encode(const LdpcEncodeParams &p, int rate, int num_cu, const Tuning *tune, hipStream_t st);
// k_ldpc_decode.  Stage mode (status_rw == nullptr): rows of n_cw code words of 640 LLRs -> K n_cw bytes, iters (optional, n_frames *
// n_cw: the iteration a code word converged at, 0 = not within max_iter).  Chain mode (status_rw, nsym, out_len required): the frame
// rule of include/ofdm_hip.h on the LLRs from 128 on; rows with status != 0 are skipped with out_len 0, status may become
// OFDM_FRAME_HEADER or OFDM_FRAME_UNCORRECTABLE.
struct LdpcDecodeParams {
    const int8_t *llr = nullptr;
    long long n_frames = 0, llr_stride = 0, n_cw = 0;
    int max_iter = 0;
    uint8_t *out = nullptr;
    long long out_stride = 0;
    int32_t *iters = nullptr;
    int32_t *status_rw = nullptr, *out_len = nullptr;
    const int32_t *nsym = nullptr;
    int bytes_per_symbol = 0;
};
hipError_t run_ldpc_decode(const LdpcDecodeParams &p, int rate, int num_cu, const Tuning *tune, hipStream_t st);
const char *ldpc_encode_name(int rate); // the dispatch name of the kernel a rate launches
const char *ldpc_decode_name(int rate);

// ---- EXT-5 channel-estimate denoising (OFDM_CHEST_WLS, ofdm_chest_smooth_batch; kernels_chest.hip, definition: tests/chest_ref.py)
// rows of n_fft bins times the per-bin weight w (a weight of exactly 0 gives 0 whatever the bin holds); in == out allowed
hipError_t run_chest_weight(const float2 *in, const float *w, float2 *out, long long n_frames, int n_fft, int num_cu, const Tuning *tune,
                            hipStream_t st);
// out row f = n_fft taps: tap (m - pre) mod n_fft = sum_n mt[n][m] g[f][(n - pre) mod n_fft] for m in [0, n_taps), every other tap 0.
// mt: the n_taps x n_taps matrix TRANSPOSED (row = contraction index).  n_fft = 4 n_taps, n_taps a multiple of 16; g != out.
struct ChestSolveParams {
    const float2 *g = nullptr;
    float2 *out = nullptr;
    const float2 *mt = nullptr;
    long long n_frames = 0;
    int n_fft = 0, n_taps = 0, pre = 0;
};
hipError_t run_chest_solve(const ChestSolveParams &p, int num_cu, const Tuning *tune, hipStream_t st);

// channel (src/channel.rs:33-74) on the GPU (kernels_bytes.hip)
struct ChannelParams {
    const float2 *tx = nullptr;
    long long n_frames = 0, tx_stride = 0, tx_len = 0;
    double snr_lin = 1000.0;
    int timing_error = 0;
    unsigned long long seed = 0;
    const int32_t *delay = nullptr;      // optional test-bench extension: per-frame placement inside the slot
    const double *f_delta_in = nullptr;  // optional test-bench extension: per-frame CFO instead of the drawn one
    float2 *out = nullptr;
    long long out_stride = 0, out_len = 0;
    double *f_delta_out = nullptr;
    int n_taps = 0;                      // the non-zero taps of CHANNEL
    int tap_idx[16] = {0};
    float tap_val[16] = {0};
};
hipError_t run_channel(const ChannelParams &p, int num_cu, hipStream_t st);

// measurement helper (ofdm_hbm_read_probe): read-only stream in k_demod64's access pattern (0), over whole symbols (1), or
// with unit-stride 16-byte loads (2)
hipError_t run_read_probe(const float2 *in, long long n_sym, int pattern, unsigned *sink, int num_cu, hipStream_t st);

} // namespace ofdm
