// ofdm_ctx.hpp -- the context behind `ofdm_ctx *` and the helpers every translation unit of the C ABI shares (internal to
// libofdm_hip.so): ofdm_abi.hip (device-buffer entry points) and ofdm_host_path.hip (host-buffer pipelines, long captures).
#pragma once
#include "../../include/ofdm_hip.h"
#include "kernels.hpp"

#include <cmath>
#include <cstddef>
#include <vector>

// ---- what a mode is.  ecc = [OFDM_ECC_FCS +] [OFDM_ECC_RS255 +] inner (include/ofdm_hip.h): the inner code makes the frames that travel,
// every outer layer turns rows (+ optional per-row lengths) into longer rows on transmit and back on receive.
enum OuterLayer { kLayerFcs, kLayerRs };
struct ModePlan {
    int n_outer = 0;
    OuterLayer outer[2] = {};   // outside-in
    int inner = OFDM_ECC_NONE;  // NONE, HAMMING74, HAMMING74_SOFT, CONV_K7, CONV_K7F_R12 / _R23 / _R34, LDPC648 or LDPC648_R23 / _R34 / _R56
    bool has(OuterLayer l) const { return (n_outer > 0 && outer[0] == l) || (n_outer > 1 && outer[1] == l); }
    // rate (0 = 1/2, 1 = 2/3, 2 = 3/4) of a framed convolutional inner mode, -1 for every other
    int rate() const { return inner >= OFDM_ECC_CONV_K7F_R12 && inner <= OFDM_ECC_CONV_K7F_R34 ? inner - OFDM_ECC_CONV_K7F_R12 : -1; }
    bool conv() const { return inner == OFDM_ECC_CONV_K7 || rate() >= 0; }
    // rate (0 = 1/2, 1 = 2/3, 2 = 3/4, 3 = 5/6) of an LDPC(648) inner mode, -1 for every other
    int ldpc_rate() const {
        if (inner == OFDM_ECC_LDPC648) return 0;
        return inner >= OFDM_ECC_LDPC648_R23 && inner <= OFDM_ECC_LDPC648_R56 ? inner - OFDM_ECC_LDPC648_R23 + 1 : -1;
    }
    bool ldpc() const { return ldpc_rate() >= 0; }
    bool soft() const { return inner == OFDM_ECC_HAMMING74_SOFT || conv() || ldpc(); } // decoded from LLRs
};
// The plan of `ecc`; false when ecc is no mode (3 and 4 are none, nor are 21 .. 29 or 36 and 61 .. 63 = RS around LDPC; 64 + a base mode
// is one).  RS goes around OFDM_ECC_NONE and the framed modes only, the frame check around all fifteen.
inline bool mode_plan(int ecc, ModePlan *m) {
    *m = ModePlan();
    if (ecc >= OFDM_ECC_FCS) { m->outer[m->n_outer++] = kLayerFcs; ecc -= OFDM_ECC_FCS; }
    const int in = ecc - OFDM_ECC_RS255;
    if (in == OFDM_ECC_NONE || (in >= OFDM_ECC_CONV_K7F_R12 && in <= OFDM_ECC_CONV_K7F_R34)) { m->outer[m->n_outer++] = kLayerRs; ecc = in; }
    m->inner = ecc;
    return ecc == OFDM_ECC_NONE || ecc == OFDM_ECC_HAMMING74 || ecc == OFDM_ECC_HAMMING74_SOFT || m->conv() || m->ldpc();
}

// The two length maps of every layer.  *_coded_bytes: payload bytes -> the bytes the layer makes of them.  *_row_limit: the largest row
// the layer can deliver for `body` bytes in front of it (inner: the bytes behind the 16-byte length header; outer: the row below).
inline int64_t inner_coded_bytes(const ModePlan &m, int64_t n) {
    if (m.inner == OFDM_ECC_CONV_K7) return 2 * (n + 1); // rate 1/2 over the payload and one tail byte
    if (m.rate() >= 0) return ofdm::kConvLengthBlock + ofdm::conv_body_len(n, m.rate());
    if (m.ldpc()) return ofdm_ldpc648_coded_len_rate(n, m.ldpc_rate());
    return m.inner != OFDM_ECC_NONE ? ((n + 3) / 4) * 7 : n; // the soft decoder reads the same code
}
inline int64_t inner_row_limit(const ModePlan &m, int64_t body) {
    if (m.inner == OFDM_ECC_NONE) return body;
    if (m.ldpc()) return body >= 80 ? ofdm_ldpc648_info_bytes(m.ldpc_rate()) * (body / 80) - 8 : 0; // the whole code words' info bytes less the two length words
    if (m.inner == OFDM_ECC_CONV_K7) return body / 2 >= 1 ? body / 2 - 1 : 0;    // 4 body steps = body / 2 bytes, less the tail byte
    if (m.rate() >= 0)                               // the steps a body cut at the end of the capture still holds, behind the length block
        return body >= ofdm::kConvLengthBlock ? ofdm::conv_max_steps(8 * (body - ofdm::kConvLengthBlock), m.rate()) / 8 : 0;
    return (body / 7) * 4;                                                       // Hamming(7,4), hard or soft
}
inline int64_t outer_coded_bytes(OuterLayer l, int64_t n) { return l == kLayerFcs ? n + OFDM_FCS_OVERHEAD : ofdm_rs255_encoded_len(n); }
// (kLayerFcs: below 0 for a row shorter than the envelope, which delivers nothing)
inline int64_t outer_row_limit(OuterLayer l, int64_t row) { return l == kLayerFcs ? row - OFDM_FCS_OVERHEAD : ofdm_rs255_decoded_len(row); }

// ... composed over the plan: what ofdm_coded_len returns, and the row size every decode entry point asks of its caller
inline int64_t coded_len(const ModePlan &m, int64_t n) {
    for (int i = 0; i < m.n_outer; i++) n = outer_coded_bytes(m.outer[i], n);
    return inner_coded_bytes(m, n);
}
inline int64_t row_bytes(const ModePlan &m, int64_t body) {
    int64_t row = inner_row_limit(m, body);
    for (int i = m.n_outer - 1; i >= 0; i--) row = outer_row_limit(m.outer[i], row);
    return row > 0 ? row : 0;
}

struct Workspace {
    void *ptr = nullptr;
    size_t cap = 0;
};
// One slot per buffer role.  The rule: two roles that can be live in the same entry point never share a slot.
enum WsRole {
    kWsDhat, kWsFdelta, kWsOffset, kWsNsym, kWsHk, kWsRaw, kWsCut, kWsLlr, kWsSurvivors, // the decode chain, search to finish
    kWsSearch, kWsSearchD1,      // the timing search's scratch (k_sc_*, k_scb_*, k_xcorr: one at a time) and the tiled search's first crossings
    kWsChestTaps,                // EXT-5: the solve's zeroed rows
    kWsRxFcsRows, kWsRxRsRows,   // decode: the dword rows an outer layer reads
    kWsBranchStatus, kWsBranchQuality, kWsCombinedNsym, // EXT-7 combine chain: per branch row status and quality rows, per frame merged live symbols
    kWsTxFcsRows, kWsTxFcsLen, kWsTxRsRows, kWsTxRsLen, kWsTxCoded, kWsTxCodedLen, // encode: rows and ragged lengths out of every layer
    kWsFrameMax,                 // per-frame maxima (ofdm_tx_encode_batch, ofdm_normalize_batch)
    kWsProbeSink,                // ofdm_hbm_read_probe
    kWsSc16,                     // EXT-9: one chunk of frames widened from sc16, the input of the fc32 path behind the sc16 entry points
    kWsTxSc16,                   // EXT-10: one chunk of fc32 frames out of the encode chain, the input of k_sc16_narrow (ofdm_tx_encode_sc16_batch)
    kWsLongSc16,                 // EXT-10: one long sc16 capture widened, the input of the fc32 long decode (ofdm_rx_decode_long_sc16[_host])
    kWsNoiseWeight,              // EXT-11: per row of the decode chain the n_fft LLR weights q_k of k_noise_bins, read by k_sym<llrw> (OFDM_LLRW_NOISE)
    kWsScanBits, kWsScanRows,    // EXT-12: ofdm_sc_scan_long's bitmap of crossings; its head {n_det, more} and the rows d1 | d_hat | f_delta | metric
    kWsPktDet, kWsPktGeom,       // EXT-13: ofdm_rx_decode_packets' uploaded detections d_hat | f_delta | metric; per packet row_start | row d_hat | row length
    kWsPktRows,                  // EXT-13: one chunk of gathered rows (R samples each), the input of the chain
    kWsPktFdelta, kWsPktOffset,  // EXT-13: per packet the chain's f_delta when the caller takes none; the chain's int32 row offsets
    kWsRoles
};

struct HostPipe; // pinned staging, copy streams and slot buffers of the host-buffer entry points (ofdm_host_path.hip)

struct ofdm_ctx {
    ofdm_params prm;
    ModePlan mode;                // the layers of prm.ecc (ofdm_create)
    int device = 0;
    int num_cu = 256;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int last_hip = 0;
    // constant device tables
    float2 *d_tw = nullptr;       // exp(-2 pi i m / N)
    float2 *d_inv_trn = nullptr;  // 1 / training[k]
    float2 *d_header = nullptr;   // 10 * S un-normalised header samples
    float header_max = 0.f;
    // EXT-5 channel-estimate denoising: built by ofdm_create when chest_mode is on, else by the first ofdm_chest_smooth_batch
    std::vector<double> training;       // the context's training table (interleaved re, im): what the tables below are made from
    float *d_chest_w = nullptr;         // W_k = |t_k|^2
    float2 *d_chest_mt = nullptr;       // N R^-1, transposed: [L_h][L_h]
    // EXT-8 wide CFO acquisition: built by ofdm_create when cfo_mode is OFDM_CFO_WIDE, else by the first ofdm_cfo_wide_batch
    float2 *d_trn = nullptr;            // training[k]
    int llr_weight = OFDM_LLRW_CHANNEL; // EXT-11 (ofdm_set_llr_weight): what the decode chains weigh their LLRs by
    ofdm::Tuning tune;                  // ofdm_set_tuning: per-context A/B switches and grid shapes (no environment variable is read)
    double sync_threshold_f64 = 0.0;    // ofdm_set_tuning "sync_threshold_bits": the packet-detect threshold as a double (0 = prm.sync_threshold, a float)
    ofdm::Trace trace;                  // ofdm_last_dispatch: the kernels the last entry point launched
    ofdm::ScStats sc_stats;             // list counters of the last Schmidl-Cox search (ofdm_get_tuning "stat_sc_*")
    int32_t *d_stats = nullptr;         // [2] their home on the device (owned by the context)
    // workspaces (grown on demand, never inside a captured region)
    Workspace ws[kWsRoles];
    int ws_poison = 0;            // ofdm_set_tuning "ws_poison" (ofdm_hip_tuning.h): 0 = off, 0x100 + b = every growth is filled with byte b
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    HostPipe *pipe = nullptr;     // created by the first host-buffer call, freed by ofdm_destroy

    int S() const { return prm.n_fft + prm.cp_len; }
    int carriers() const { return prm.guard_bands ? 48 * (prm.n_fft / 64) : prm.n_fft; }
    int bytes_per_symbol() const { return carriers() * prm.modulation / 8; }
};

// Scoped device selection: every entry point that touches HIP runs on its context's device and leaves the calling
// thread's current device as it found it (one thread may hold contexts on several GPUs; torch shares the thread's device).
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(int device) {
        if (hipGetDevice(&prev) == hipSuccess && prev != device) switched = hipSetDevice(device) == hipSuccess;
    }
    ~DeviceGuard() { if (switched) hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};
// The scope of an entry point that launches kernels: the context's device, and an empty dispatch trace.  The one place the trace is
// reset: everything below an entry point appends to it in launch order (Trace, kernels.hpp).
struct EntryScope {
    DeviceGuard dev;
    explicit EntryScope(ofdm_ctx *c) : dev(c->device) { c->trace.reset(); }
};

#define HIP_TRY(ctx, expr)                                   \
    do {                                                     \
        hipError_t _e = (expr);                              \
        if (_e != hipSuccess) { (ctx)->last_hip = (int)_e; return OFDM_ERR_HIP; } \
    } while (0)

// "ws_poison" (ofdm_hip_tuning.h): fill a fresh device allocation over its whole capacity before any kernel or copy of any stream sees it
inline int poison_fill_dev(ofdm_ctx *c, void *p, size_t cap, int fill) {
    HIP_TRY(c, hipMemsetAsync(p, fill, cap, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return OFDM_OK;
}

inline int ws_get(ofdm_ctx *c, WsRole role, size_t bytes, void **out) {
    Workspace &w = c->ws[role];
    if (bytes > w.cap) {
        if (w.ptr) { HIP_TRY(c, hipStreamSynchronize(c->stream)); HIP_TRY(c, hipFree(w.ptr)); w.ptr = nullptr; w.cap = 0; }
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&w.ptr, want);
        if (e != hipSuccess) { c->last_hip = (int)e; w.ptr = nullptr; return OFDM_ERR_NOMEM; }
        w.cap = want;
        if (c->ws_poison) { const int rc = poison_fill_dev(c, w.ptr, want, c->ws_poison & 0xFF); if (rc) return rc; }
    }
    *out = w.ptr;
    return OFDM_OK;
}

// ---- rules both translation units spell the same way
inline bool sc16_scale_ok(float scale) { return std::isfinite(scale) && scale > 0.f; }
// The bytes behind the 16-byte length header of max_symbols demodulated symbols, and the row size every decode entry point asks of its
// caller for them (include/ofdm_hip.h)
inline int64_t decode_body_bytes(const ofdm_ctx *c, int32_t max_symbols) {
    const int64_t raw = (int64_t)max_symbols * c->bytes_per_symbol();
    return raw > 16 ? raw - 16 : 0;
}
inline int64_t decode_row_bytes(const ofdm_ctx *c, int32_t max_symbols) { return row_bytes(c->mode, decode_body_bytes(c, max_symbols)); }
// k_sc16_widen / k_sc16_narrow over n_frames rows of frame_len samples; the caller adds the two pointers of its direction
inline ofdm::Sc16Params sc16_params(ofdm_ctx *c, int64_t n_frames, int64_t frame_len, int64_t in_stride, int64_t out_stride, float scale) {
    ofdm::Sc16Params p;
    p.tune = &c->tune; p.trace = &c->trace;
    p.n_frames = n_frames; p.frame_len = frame_len; p.in_stride = in_stride; p.out_stride = out_stride; p.scale = scale;
    return p;
}

// ---- packed records: the blocks that travel between device, pinned memory and caller as ONE allocation or copy.  A layout is a struct
// whose constructor takes its columns from a Carver in order; built on no memory (base = nullptr) the same walk gives the size alone.
struct Carver {
    char *base;
    size_t at = 0; // bytes taken so far
    explicit Carver(const void *b) : base(static_cast<char *>(const_cast<void *>(b))) {}
    // the next column: n entries of T, on T's alignment (or the larger `align`, a power of two)
    template <class T> T *col(size_t n, size_t align = alignof(T)) {
        at = (at + align - 1) & ~(align - 1);
        T *p = base ? reinterpret_cast<T *>(base + at) : nullptr;
        at += n * sizeof(T);
        return p;
    }
};
// what a decode call leaves per frame: the pipe's device and bounce slots (ofdm_rx_decode_host), the one frame of ofdm_rx_decode_long
struct DecodeBlock {
    double *f_delta; int32_t *len, *status, *offset; float *metric; uint8_t *rows; size_t bytes;
    DecodeBlock(const void *base, size_t n, size_t row_bytes) {
        Carver k(base);
        f_delta = k.col<double>(n); len = k.col<int32_t>(n); status = k.col<int32_t>(n); offset = k.col<int32_t>(n); metric = k.col<float>(n);
        rows = k.col<uint8_t>(n * row_bytes);
        bytes = k.at;
    }
};
// ... per packet (ofdm_rx_decode_all_long_host): the offsets are 64-bit, the rows start on 16 bytes
struct PacketsBlock {
    int64_t *offset; double *f_delta; int32_t *len, *status; float *metric; uint8_t *rows; size_t bytes;
    PacketsBlock(const void *base, size_t n, size_t row_bytes) {
        Carver k(base);
        offset = k.col<int64_t>(n); f_delta = k.col<double>(n); len = k.col<int32_t>(n); status = k.col<int32_t>(n); metric = k.col<float>(n);
        rows = k.col<uint8_t>(n * row_bytes, 16);
        bytes = k.at;
    }
};
// ofdm_sc_scan_long's result (kWsScanRows and its pinned copy): the head {n_det, more}, then `cap` entries a column
struct ScanRows {
    long long *head, *d1, *d_hat; double *f_delta; float *metric; size_t bytes;
    ScanRows(const void *base, size_t cap) {
        Carver k(base);
        head = k.col<long long>(2); d1 = k.col<long long>(cap); d_hat = k.col<long long>(cap); f_delta = k.col<double>(cap); metric = k.col<float>(cap);
        bytes = k.at;
    }
};
// ofdm_rx_decode_packets: the uploaded detections (kWsPktDet) and what k_pkt_rows makes of them (kWsPktGeom)
struct PktDetections {
    long long *d_hat; double *f_delta; float *metric; size_t bytes;
    PktDetections(const void *base, size_t n) {
        Carver k(base);
        d_hat = k.col<long long>(n); f_delta = k.col<double>(n); metric = k.col<float>(n);
        bytes = k.at;
    }
};
struct PktGeometry {
    long long *row_start; int32_t *row_dhat, *row_len; size_t bytes;
    PktGeometry(const void *base, size_t n) {
        Carver k(base);
        row_start = k.col<long long>(n); row_dhat = k.col<int32_t>(n); row_len = k.col<int32_t>(n);
        bytes = k.at;
    }
};
// the long search's per-slice detector outputs (HostPipe::d_scal)
struct SliceRows {
    double *f_delta; int32_t *d_hat; float *metric; size_t bytes;
    SliceRows(const void *base, size_t n) {
        Carver k(base);
        f_delta = k.col<double>(n); d_hat = k.col<int32_t>(n); metric = k.col<float>(n);
        bytes = k.at;
    }
};

// ---- a decode call, as the chain takes it (ofdm_abi.hip)
// Timing the caller brings.  One capture: d_hat / f_delta / metric by value (ofdm_rx_decode_long with lag_lo > 0).  Rows (EXT-13,
// row_dhat != NULL): device arrays of the row-relative peaks and of the rows' own lengths; the call's f_delta and offset arrays are not
// optional, f_delta (and metric, if wanted) already hold the rows' values
struct KnownSync { int32_t d_hat; double f_delta; float metric; const int32_t *row_dhat = nullptr, *row_len = nullptr; };
// The arguments of a decode call: ofdm_rx_decode_batch's own, or captures with their timing
struct DecodeCall {
    const float2 *in; int64_t n_frames, frame_stride, frame_len, n_lags; int32_t max_symbols;
    uint8_t *out; int64_t out_stride;                          // rows of out_stride bytes
    int32_t *out_len, *status, *offset; double *f_delta; float *metric; // per frame (offset, f_delta, metric: optional)
    const KnownSync *known;
};

// internal cross-file helpers (C linkage only because their definitions sit inside the extern "C" blocks; not in ofdm_hip.h)
extern "C" {
__attribute__((visibility("hidden"))) void ofdm_host_pipe_destroy(ofdm_ctx *c); // ofdm_host_path.hip; the context's device is current
// "ws_poison" set on (ofdm_host_path.hip; the context's device is current): synchronise the pipe's streams, if a pipe exists, and fill
// every device and pinned buffer it holds over its whole capacity with the byte `fill`
__attribute__((visibility("hidden"))) int ofdm_host_pipe_poison(ofdm_ctx *c, int fill);
// "stat_pipe_*": buffer i of the pipe (no pipe yet: nullptr, 0) and whether it is pinned host memory; 0 behind the last buffer
__attribute__((visibility("hidden"))) int ofdm_host_pipe_buffer(const ofdm_ctx *c, int i, void **p, size_t *cap, int *pinned);
// Schmidl-Cox over a batch (the dispatcher behind ofdm_sc_correlate_batch and step 1 of ofdm_rx_decode_batch; ofdm_abi.hip)
__attribute__((visibility("hidden"))) int ofdm_abi_sc_run(ofdm_ctx *c, const float2 *in, int64_t n_frames, int64_t frame_stride, int64_t frame_len, int64_t n_lags,
                    int32_t *d_hat, double *f_delta, float *metric);
// ofdm_rx_decode_batch behind its entry scope: the argument checks and the chain of d, appended to the context's trace (the long
// capture calls run it on a sub-capture, with the chain's own search or, d.known, with the slice search's timing)
__attribute__((visibility("hidden"))) int ofdm_abi_rx_decode(ofdm_ctx *c, const DecodeCall &d);
// EXT-13 (ofdm_rx_decode_packets behind its argument checks and its entry scope: ofdm_rx_decode_all_long_host runs it behind its scan).
// n_whole (0: n): the samples of the capture whose last n samples `in` holds (EXT-14: a stream's window).  Only the row length R is taken
// from it, so that a window's rows are, zeros included, the rows of the whole capture
__attribute__((visibility("hidden"))) int ofdm_abi_rx_decode_packets(ofdm_ctx *c, const float2 *in, int64_t n, int64_t n_det, const int64_t *d_hat,
                    const double *f_delta, const float *metric, int32_t max_symbols, uint8_t *out, int64_t out_stride, int32_t *out_len,
                    int32_t *status, int64_t *offset, double *f_delta_out, float *metric_out, int64_t n_whole);
}
