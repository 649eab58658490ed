// ofdm_ctx.hpp -- the context behind `ofdm_ctx *` and the helpers every translation unit of the C ABI shares (internal to
// libofdm_hip.so): ofdm_abi.hip (device-buffer entry points) and ofdm_host_path.hip (host-buffer pipelines, long captures).
#pragma once
#include "../../include/ofdm_hip.h"
#include "kernels.hpp"

#include <cstddef>
#include <vector>

struct Workspace {
    void *ptr = nullptr;
    size_t cap = 0;
};

struct HostPipe; // pinned staging, copy streams and slot buffers of the host-buffer entry points (ofdm_host_path.hip)

struct ofdm_ctx {
    ofdm_params prm;
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
    ofdm::Tuning tune;                  // ofdm_set_tuning: per-context A/B switches and grid shapes (no environment variable is read)
    ofdm::Trace trace;                  // ofdm_last_dispatch: the kernels the last entry point launched
    ofdm::ScStats sc_stats;             // list counters of the last Schmidl-Cox search (ofdm_get_tuning "stat_sc_*")
    int32_t *d_stats = nullptr;         // [2] their home on the device (owned by the context)
    // workspaces (grown on demand, never inside a captured region)
    Workspace ws[16];
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

#define HIP_TRY(ctx, expr)                                   \
    do {                                                     \
        hipError_t _e = (expr);                              \
        if (_e != hipSuccess) { (ctx)->last_hip = (int)_e; return OFDM_ERR_HIP; } \
    } while (0)

inline int ws_get(ofdm_ctx *c, int slot, size_t bytes, void **out) {
    Workspace &w = c->ws[slot];
    if (bytes > w.cap) {
        if (w.ptr) { HIP_TRY(c, hipStreamSynchronize(c->stream)); HIP_TRY(c, hipFree(w.ptr)); w.ptr = nullptr; w.cap = 0; }
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&w.ptr, want);
        if (e != hipSuccess) { c->last_hip = (int)e; w.ptr = nullptr; return OFDM_ERR_NOMEM; }
        w.cap = want;
    }
    *out = w.ptr;
    return OFDM_OK;
}

// rate (0 = 1/2, 1 = 2/3, 2 = 3/4) of a framed convolutional mode, -1 for every other ecc value
inline int framed_rate(int ecc) { return ecc >= OFDM_ECC_CONV_K7F_R12 && ecc <= OFDM_ECC_CONV_K7F_R34 ? ecc - OFDM_ECC_CONV_K7F_R12 : -1; }

// OFDM_ECC_RS255* = 20 + inner: the outer Reed-Solomon code around the frames of the inner mode (OFDM_ECC_NONE or a framed mode)
inline bool rs_outer(int ecc) { return ecc == OFDM_ECC_RS255 || (ecc >= OFDM_ECC_RS255_K7F_R12 && ecc <= OFDM_ECC_RS255_K7F_R34); }
// the mode whose frames travel: ecc itself, or the inner mode of an RS mode
inline int inner_ecc(int ecc) { return rs_outer(ecc) ? ecc - OFDM_ECC_RS255 : ecc; }

// OFDM_ECC_FCS + mode = 64 + mode: the CRC-32 frame check around the frames of `mode`, any of the twelve base modes (an RS mode included)
inline bool base_mode(int ecc) {
    return ecc == OFDM_ECC_NONE || ecc == OFDM_ECC_HAMMING74 || ecc == OFDM_ECC_HAMMING74_SOFT || ecc == OFDM_ECC_CONV_K7 || framed_rate(ecc) >= 0 ||
           rs_outer(ecc) || ecc == OFDM_ECC_LDPC648;
}
inline bool fcs_outer(int ecc) { return ecc >= OFDM_ECC_FCS && base_mode(ecc - OFDM_ECC_FCS); }
// the mode whose frames carry the envelope: ecc itself, or the base mode of an FCS mode
inline int base_ecc(int ecc) { return fcs_outer(ecc) ? ecc - OFDM_ECC_FCS : ecc; }

// Largest out_len the decode chain of mode `ecc` (no RS mode) can write for a frame whose body (the bytes behind the 16-byte length
// header) is `body` bytes
inline int64_t inner_row_bytes(int ecc, int64_t body) {
    if (ecc == OFDM_ECC_NONE) return body;
    if (ecc == OFDM_ECC_LDPC648) return body >= 80 ? 40 * (body / 80) - 8 : 0; // the whole code words' info bytes less the two length words
    if (ecc == OFDM_ECC_CONV_K7) return body / 2 >= 1 ? body / 2 - 1 : 0; // 4 body steps = body / 2 bytes, less the tail byte
    if (framed_rate(ecc) >= 0)                       // the steps a body cut at the end of the capture still holds, behind the length block
        return body >= ofdm::kConvLengthBlock ? ofdm::conv_max_steps(8 * (body - ofdm::kConvLengthBlock), framed_rate(ecc)) / 8 : 0;
    return (body / 7) * 4;                                                       // Hamming(7,4), hard or soft
}
// ... of base mode `ecc` (no FCS mode).  RS modes: the decoded blocks of the longest row the inner mode can deliver.
inline int64_t base_row_bytes(int ecc, int64_t body) {
    const int64_t inner = inner_row_bytes(inner_ecc(ecc), body);
    return rs_outer(ecc) ? ofdm_rs255_decoded_len(inner) : inner;
}
// ... of the context's mode: the row size every decode entry point asks of its caller (include/ofdm_hip.h).  FCS modes: the base
// mode's row less the envelope's 8 bytes.
inline int64_t decode_row_bytes(const ofdm_ctx *c, int64_t body) {
    const int64_t base = base_row_bytes(base_ecc(c->prm.ecc), body);
    return fcs_outer(c->prm.ecc) ? (base > OFDM_FCS_OVERHEAD ? base - OFDM_FCS_OVERHEAD : 0) : base;
}

// internal cross-file helpers (C linkage only because their definitions sit inside the extern "C" blocks; not in ofdm_hip.h)
extern "C" {
__attribute__((visibility("hidden"))) void ofdm_host_pipe_destroy(ofdm_ctx *c); // ofdm_host_path.hip; the context's device is current
// Schmidl-Cox over a batch (the dispatcher behind ofdm_sc_correlate_batch and step 1 of ofdm_rx_decode_batch; ofdm_abi.hip)
__attribute__((visibility("hidden"))) int ofdm_abi_sc_run(ofdm_ctx *c, const float2 *in, int64_t n_frames, int64_t frame_stride, int64_t frame_len, int64_t n_lags,
                    int32_t *d_hat, double *f_delta, float *metric);
// ofdm_rx_decode_batch for ONE capture whose timing is already known (peak lag d_hat, arg P / L and metric at it): steps 2-5 of the
// chain without its own search (ofdm_rx_decode_long with lag_lo > 0: the search must not look at lags in front of lag_lo)
__attribute__((visibility("hidden"))) int ofdm_abi_rx_decode_known(ofdm_ctx *c, const ofdm_fc32 *in, int64_t frame_len, int32_t d_hat, double f_delta, float metric,
                    int32_t max_symbols, uint8_t *out, int64_t out_stride, int32_t *out_len, int32_t *status, int32_t *offset, double *f_delta_out,
                    float *metric_out);
}
