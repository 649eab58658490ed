// ofdm_host.hpp -- C++ host-side mirror of the reference's TX/RX function surface over the C ABI (ofdm_hip.h).
//
// The reference crate exposes free functions (src/lib.rs:8-21): encode, decode, modulate, demodulate, prefix_block,
// unprefix_block, ... on Vec<Complex64>.  This header keeps those names, argument meanings, defaults and error
// behaviour for a C++ host: std::vector<std::complex<double>> in and out, conversion to the fc32 wire format at the
// boundary (utils::sig_to_bytes / bytes_to_sig, src/utils.rs:228-254), device staging through ofdm_dev_alloc /
// ofdm_memcpy_*.  Header-only; link with -lofdm_hip.  Errors: decode returns the reference's
// "Input not long enough, bailing early" (src/receiver.rs:27-29) as a std::runtime_error, as anyhow::Result does.
#pragma once
#include "ofdm_hip.h"

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

namespace ofdm {

using Complex64 = std::complex<double>;
enum class ModulationScheme { Bpsk = OFDM_MOD_BPSK, Qpsk = OFDM_MOD_QPSK, Qam16 = OFDM_MOD_QAM16, Qam64 = OFDM_MOD_QAM64, Qam256 = OFDM_MOD_QAM256 };

struct Error : std::runtime_error { using std::runtime_error::runtime_error; };

inline void check(int rc, const char *what) {
    if (rc != OFDM_OK) throw Error(std::string(what) + ": " + ofdm_strerror(rc));
}

// RAII context = one (thread, GPU) handle
// which preamble / training tables a context is built with (src/transmitter.rs:75-96)
enum class Pilots {
    Default, // documented SplitMix64 draws (ofdm_default_pilots)
    StdRng,  // the reference's own rand 0.8 StdRng draws, restated and unverified (ofdm_stdrng_pilots)
};
inline Pilots &default_pilot_choice() { static Pilots p = Pilots::Default; return p; } // used by the free encode / decode

class Context {
  public:
    explicit Context(bool guard_bands = false, ModulationScheme m = ModulationScheme::Bpsk, int n_fft = 64,
                     int ecc = OFDM_ECC_NONE, int cfo_mode = OFDM_CFO_SIGNED, int device = 0,
                     Pilots pilots = default_pilot_choice(), int chest_mode = OFDM_CHEST_LS) {
        ofdm_params p;
        check(ofdm_default_params(&p), "ofdm_default_params");
        p.n_fft = n_fft; p.cp_len = n_fft / 4; p.guard_bands = guard_bands; p.modulation = (int)m; p.ecc = ecc; p.cfo_mode = cfo_mode;
        p.chest_mode = chest_mode; // OFDM_CHEST_WLS: decode works with the denoised channel estimate (include/ofdm_hip.h, EXT-5)
        n_fft_ = n_fft;
        ecc_ = ecc;
        window_reps_ = p.sync_window_reps;
        if (pilots == Pilots::StdRng) {
            std::vector<double> pre(2 * (size_t)(n_fft + n_fft / 4)), trn(2 * (size_t)n_fft);
            check(ofdm_stdrng_pilots(n_fft, n_fft / 4, pre.data(), trn.data()), "ofdm_stdrng_pilots");
            check(ofdm_create(&p, pre.data(), trn.data(), device, nullptr, &ctx_), "ofdm_create");
        } else {
            check(ofdm_create(&p, nullptr, nullptr, device, nullptr, &ctx_), "ofdm_create");
        }
    }
    ~Context() { ofdm_destroy(ctx_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    ofdm_ctx *raw() const { return ctx_; }
    int symbol_len() const { return ofdm_symbol_len(ctx_); }

    struct DevBuf { // device allocation tied to the context
        ofdm_ctx *c; void *p = nullptr;
        DevBuf(ofdm_ctx *ctx, size_t bytes) : c(ctx) { check(ofdm_dev_alloc(c, bytes ? bytes : 1, &p), "ofdm_dev_alloc"); }
        ~DevBuf() { ofdm_dev_free(c, p); }
        DevBuf(const DevBuf &) = delete;
    };
    static std::vector<ofdm_fc32> to_fc32(const std::vector<Complex64> &x) { // sig_to_bytes (src/utils.rs:228-236)
        std::vector<ofdm_fc32> o(x.size());
        for (size_t i = 0; i < x.size(); ++i) o[i] = ofdm_fc32{(float)x[i].real(), (float)x[i].imag()};
        return o;
    }
    static std::vector<Complex64> from_fc32(const std::vector<ofdm_fc32> &x) { // bytes_to_sig (src/utils.rs:238-254)
        std::vector<Complex64> o(x.size());
        for (size_t i = 0; i < x.size(); ++i) o[i] = Complex64(x[i].re, x[i].im);
        return o;
    }

    // encode (src/transmitter.rs:11-58): host bytes in, host samples out (ofdm_tx_encode_host does the staging)
    std::vector<Complex64> encode(const std::vector<uint8_t> &data) {
        const int64_t n = ofdm_frame_samples(ctx_, (int64_t)data.size());
        std::vector<ofdm_fc32> host((size_t)n);
        const uint8_t none = 0;
        check(ofdm_tx_encode_host(ctx_, data.empty() ? &none : data.data(), 1, (int64_t)data.size(), nullptr, (int32_t)data.size(),
                                  host.data(), n, 0), "ofdm_tx_encode_host");
        return from_fc32(host);
    }
    // EXT-10: the same frame as sc16 for a DAC (ofdm_tx_encode_sc16_host): ofdm_sc16_narrow(encode(data), scale), made on the device and
    // brought back at 4 bytes a sample.  *clipped (optional): components that clipped -- a normalised frame's negative peak is not
    // bounded by -1 (include/ofdm_hip.h), so a count above 0 means the scale is too large for this frame.
    std::vector<ofdm_sc16> encode_sc16(const std::vector<uint8_t> &data, float scale, int32_t *clipped = nullptr) {
        const int64_t n = ofdm_frame_samples(ctx_, (int64_t)data.size());
        std::vector<ofdm_sc16> host((size_t)n);
        const uint8_t none = 0;
        check(ofdm_tx_encode_sc16_host(ctx_, data.empty() ? &none : data.data(), 1, (int64_t)data.size(), nullptr, (int32_t)data.size(), scale,
                                       host.data(), n, clipped, 0), "ofdm_tx_encode_sc16_host");
        return host;
    }
    // decode (src/receiver.rs:9-96) of ONE capture of any length -- the 2 M-sample buffers of examples/jetson_rx.rs:15-17,84-86
    // included: ofdm_rx_decode_long_host searches a long capture as a batch of overlapping slices.  Takes the samples by value
    // like the reference (which consumes its Vec).  max_symbols <= 0: every symbol up to the capture's end, as the reference.
    struct Decoded { std::vector<uint8_t> bytes; int32_t status = 0; int64_t offset = 0; double f_delta = 0.0; float metric = 0.f; };
    Decoded decode_capture(const ofdm_fc32 *fc, int64_t n, int32_t max_symbols = 0) {
        return decode_capture_as(n, max_symbols, [&](int32_t ms, Decoded &r, int64_t ob, int32_t *len) {
            check(ofdm_rx_decode_long_host(ctx_, fc, n, ms, r.bytes.data(), ob, len, &r.status, &r.offset, &r.f_delta, &r.metric),
                  "ofdm_rx_decode_long_host");
        });
    }
    // EXT-10: the same of an sc16 capture as a radio delivers it (ofdm_rx_decode_long_sc16_host): half the bytes over the link, the
    // result of decode_capture on ofdm_sc16_widen(capture, scale)
    Decoded decode_capture_sc16(const ofdm_sc16 *sc, int64_t n, int32_t max_symbols = 0, float scale = OFDM_SC16_DEFAULT_SCALE) {
        return decode_capture_as(n, max_symbols, [&](int32_t ms, Decoded &r, int64_t ob, int32_t *len) {
            check(ofdm_rx_decode_long_sc16_host(ctx_, sc, n, scale, ms, r.bytes.data(), ob, len, &r.status, &r.offset, &r.f_delta, &r.metric),
                  "ofdm_rx_decode_long_sc16_host");
        });
    }
    template <class Call> Decoded decode_capture_as(int64_t n, int32_t max_symbols, Call &&call) { // the row both calls size the same way
        const int S = symbol_len();
        if (max_symbols <= 0) max_symbols = (int32_t)std::max<int64_t>((n + S - 1) / S - 10, 1);
        int64_t ob = std::max<int64_t>((int64_t)max_symbols * ofdm_bytes_per_symbol(ctx_), 4);
        if (rs_outer(base_ecc(ecc_))) ob = ofdm_rs255_decoded_len(ob); // whole 223-byte blocks of the longest body, the trailing zero block included
        // (OFDM_ECC_FCS + mode asks for 8 bytes less than mode: the row above is large enough)
        Decoded r;
        r.bytes.resize((size_t)ob);
        int32_t len = 0;
        call(max_symbols, r, ob, &len);
        r.bytes.resize(r.status == OFDM_FRAME_OK ? (size_t)len : 0);
        return r;
    }
    std::vector<uint8_t> decode(std::vector<Complex64> samples, int32_t max_symbols = 0) {
        const auto fc = to_fc32(samples);
        return bytes_or_throw(decode_capture(fc.data(), (int64_t)fc.size(), max_symbols));
    }
    // EXT-10: decode of an sc16 capture (x = int16 * scale, widened on the device)
    std::vector<uint8_t> decode_sc16(const std::vector<ofdm_sc16> &samples, int32_t max_symbols = 0, float scale = OFDM_SC16_DEFAULT_SCALE) {
        return bytes_or_throw(decode_capture_sc16(samples.data(), (int64_t)samples.size(), max_symbols, scale));
    }
    // EXT-12: every detection of one long capture under the holdoff rule (ofdm_sc_scan_long_host, include/ofdm_hip.h): detection k has
    // its first crossing at d1[k] and its peak at d_hat[k]; the search for it started at lo(k).  more: max_det stopped the scan.
    struct Detections {
        std::vector<int64_t> d1, d_hat; std::vector<double> f_delta; std::vector<float> metric;
        int64_t lag_lo = 0, holdoff = 1; bool more = false;
        size_t size() const { return d_hat.size(); }
        int64_t lo(size_t k) const { return k ? d1[k - 1] + holdoff : lag_lo; }
    };
    Detections scan_capture(const ofdm_fc32 *fc, int64_t n, int64_t holdoff, int64_t max_det, int64_t lag_lo = 0, int64_t lag_hi = 0) {
        Detections r;
        scan_sized(r, holdoff, max_det, lag_lo, [&](int64_t *nd, int32_t *more) {
            check(ofdm_sc_scan_long_host(ctx_, fc, n, lag_lo, lag_hi, holdoff, max_det, r.d1.data(), r.d_hat.data(), r.f_delta.data(),
                                         r.metric.data(), nd, more), "ofdm_sc_scan_long_host");
        });
        return r;
    }
    // the shortest frame's holdoff: 11 S - W, at least 1 (a header and one data symbol; pass frame_samples(payload) - W for fixed-size frames)
    int64_t default_holdoff() const { return std::max<int64_t>((int64_t)(11 - window_reps_) * symbol_len(), 1); }
    // Every packet of one long capture: one upload, one scan, then ofdm_rx_decode_long(lag_lo = lo(k)) per detection.  Nothing is thrown
    // for a packet that fails: its status is in the result (a false detection inside a payload shows as OFDM_FRAME_HEADER /
    // OFDM_FRAME_FCS in the framed, LDPC and frame-check modes).  holdoff <= 0: default_holdoff().  max_symbols: the data symbols of the
    // longest frame expected (<= 0: up to the capture's end, as decode_capture -- a demod of everything behind every packet).
    // batched (EXT-13): the detections go through ONE run of the receive chain (decode_packets) instead of one ofdm_rx_decode_long each;
    // it needs max_symbols > 0 (the default "up to the capture's end" would gather the capture once per packet).  Its f_delta is the
    // scan's (within 1e-9 of the loop's), everything else is the loop's.
    std::vector<Decoded> decode_all(const ofdm_fc32 *fc, int64_t n, int64_t holdoff = 0, int64_t max_packets = 4096, int32_t max_symbols = 0,
                                    bool batched = false) {
        if (batched && max_symbols <= 0) throw Error("decode_all(batched): max_symbols is required");
        if (holdoff <= 0) holdoff = default_holdoff();
        DevBuf din(ctx_, (size_t)std::max<int64_t>(n, 1) * sizeof(ofdm_fc32) + 64);
        if (n > 0) check(ofdm_memcpy_h2d(ctx_, din.p, fc, (size_t)n * sizeof(ofdm_fc32)), "h2d");
        Detections det;
        scan_sized(det, holdoff, max_packets, 0, [&](int64_t *nd, int32_t *more) {
            check(ofdm_sc_scan_long(ctx_, (const ofdm_fc32 *)din.p, n, 0, 0, holdoff, max_packets, det.d1.data(), det.d_hat.data(),
                                    det.f_delta.data(), det.metric.data(), nd, more), "ofdm_sc_scan_long");
        });
        if (batched) return decode_packets((const ofdm_fc32 *)din.p, n, det, max_symbols);
        std::vector<Decoded> out;
        for (size_t k = 0; k < det.size(); ++k)
            out.push_back(decode_capture_as(n, max_symbols, [&](int32_t ms, Decoded &r, int64_t ob, int32_t *len) {
                DevBuf dout(ctx_, (size_t)ob + 64);
                check(ofdm_rx_decode_long(ctx_, (const ofdm_fc32 *)din.p, n, det.lo(k), 0, -1, ms, (uint8_t *)dout.p, ob, len, &r.status, &r.offset,
                                          &r.f_delta, &r.metric), "ofdm_rx_decode_long");
                if (r.status == OFDM_FRAME_OK && *len > 0) check(ofdm_memcpy_d2h(ctx_, r.bytes.data(), dout.p, (size_t)*len), "d2h");
            }));
        return out;
    }
    // EXT-13: every detection of `det` (as scan_capture / ofdm_sc_scan_long returned it) of the capture in_dev[0 .. n) on the device, in
    // one run of the receive chain (ofdm_rx_decode_packets): packet k's bytes, status, offset into the capture, the f_delta the chain
    // derotated with and the scan's metric.  Nothing is thrown for a packet that fails.
    std::vector<Decoded> decode_packets(const ofdm_fc32 *in_dev, int64_t n, const Detections &det, int32_t max_symbols) {
        const size_t nd = det.size();
        std::vector<Decoded> out(nd);
        if (!nd) return out;
        int64_t ob = 0;
        decode_capture_as(n, max_symbols, [&](int32_t, Decoded &r, int64_t row, int32_t *) { ob = row; r.status = OFDM_FRAME_NOSYNC; });
        DevBuf rows(ctx_, nd * (size_t)ob + 64), scal(ctx_, nd * 28 + 64);
        char *sp = (char *)scal.p; // offset i64 | f_delta f64 | len | status i32 | metric f32
        check(ofdm_rx_decode_packets(ctx_, in_dev, n, (int64_t)nd, det.d_hat.data(), det.f_delta.data(), det.metric.data(), max_symbols,
                                     (uint8_t *)rows.p, ob, (int32_t *)(sp + 16 * nd), (int32_t *)(sp + 20 * nd), (int64_t *)sp,
                                     (double *)(sp + 8 * nd), (float *)(sp + 24 * nd)), "ofdm_rx_decode_packets");
        std::vector<char> h(nd * 28);
        std::vector<uint8_t> b(nd * (size_t)ob);
        check(ofdm_memcpy_d2h(ctx_, h.data(), sp, h.size()), "d2h");
        check(ofdm_memcpy_d2h(ctx_, b.data(), rows.p, b.size()), "d2h");
        for (size_t k = 0; k < nd; ++k) {
            Decoded &r = out[k];
            int32_t len = 0;
            std::memcpy(&r.offset, h.data() + 8 * k, 8); std::memcpy(&r.f_delta, h.data() + 8 * nd + 8 * k, 8);
            std::memcpy(&len, h.data() + 16 * nd + 4 * k, 4); std::memcpy(&r.status, h.data() + 20 * nd + 4 * k, 4);
            std::memcpy(&r.metric, h.data() + 24 * nd + 4 * k, 4);
            if (r.status == OFDM_FRAME_OK && len > 0) r.bytes.assign(b.begin() + k * (size_t)ob, b.begin() + k * (size_t)ob + len);
        }
        return out;
    }
    template <class Call> void scan_sized(Detections &r, int64_t holdoff, int64_t max_det, int64_t lag_lo, Call &&call) {
        const size_t cap = (size_t)std::max<int64_t>(max_det, 1);
        r.d1.resize(cap); r.d_hat.resize(cap); r.f_delta.resize(cap); r.metric.resize(cap);
        r.lag_lo = lag_lo; r.holdoff = holdoff;
        int64_t nd = 0; int32_t more = 0;
        call(&nd, &more);
        r.d1.resize((size_t)nd); r.d_hat.resize((size_t)nd); r.f_delta.resize((size_t)nd); r.metric.resize((size_t)nd);
        r.more = more != 0;
    }
    static std::vector<uint8_t> bytes_or_throw(Decoded r) { // the reference's Err / None as exceptions
        if (r.status == OFDM_FRAME_SHORT) throw Error("Input not long enough, bailing early"); // src/receiver.rs:27-29
        if (r.status == OFDM_FRAME_UNCORRECTABLE) throw Error("uncorrectable block"); // RS: the reference returns None; LDPC: a code word did not converge
        if (r.status == OFDM_FRAME_FCS) throw Error("frame check failed: the payload is damaged"); // OFDM_ECC_FCS + mode
        if (r.status != OFDM_FRAME_OK) throw Error("decode failed, frame status " + std::to_string(r.status));
        return std::move(r.bytes);
    }
    // link quality (EXT-6, include/ofdm_hip.h) of the capture decode_capture just decoded: noise variance, gain, SNR and LLR unit from the
    // frame's five training blocks, and -- when payload_bytes (the size of the payload that was sent) is given -- the decision-directed
    // EVM over the points that carry it.  One channel estimate (the context's chest_mode) and one ofdm_rx_quality_batch over the frame at
    // r.offset with r.f_delta; decode itself is untouched.  A capture that was not decoded (r.status != OFDM_FRAME_OK) gives valid = false.
    struct LinkQuality { bool valid = false; float noise_var = 0.f, gain = 0.f, snr_db = NAN, llr_unit = 0.f, evm_db = NAN, points = 0.f; };
    LinkQuality link_quality(const ofdm_fc32 *fc, int64_t n, const Decoded &r, int64_t payload_bytes = -1) {
        LinkQuality q;
        if (r.status != OFDM_FRAME_OK || r.offset < 0 || r.offset >= n) return q;
        const int S = symbol_len(), nd = ofdm_data_carriers(ctx_), bps = 8 * ofdm_bytes_per_symbol(ctx_) / nd;
        int32_t points = 0, syms = 0;
        if (payload_bytes >= 0) {
            points = (int32_t)((8 * (16 + ofdm_coded_len(ctx_, payload_bytes)) + bps - 1) / bps); // the 16-byte length header included
            syms = (points + nd - 1) / nd;
        }
        const int64_t len = std::min<int64_t>(n - r.offset, (int64_t)(10 + syms) * S); // the frame alone: sample ids count from its start
        DevBuf din(ctx_, (size_t)len * sizeof(ofdm_fc32)), dhk(ctx_, (size_t)n_fft_ * sizeof(ofdm_fc32)), dfd(ctx_, sizeof(double)),
            dpts(ctx_, sizeof(int32_t)), dq(ctx_, OFDM_QUALITY_FIELDS * sizeof(float));
        check(ofdm_memcpy_h2d(ctx_, din.p, fc + r.offset, (size_t)len * sizeof(ofdm_fc32)), "h2d");
        check(ofdm_memcpy_h2d(ctx_, dfd.p, &r.f_delta, sizeof(double)), "h2d");
        check(ofdm_memcpy_h2d(ctx_, dpts.p, &points, sizeof(int32_t)), "h2d");
        check(ofdm_estimate_channel_batch(ctx_, (const ofdm_fc32 *)din.p, 1, len, len, nullptr, (const double *)dfd.p, (ofdm_fc32 *)dhk.p),
              "ofdm_estimate_channel_batch");
        check(ofdm_rx_quality_batch(ctx_, (const ofdm_fc32 *)din.p, 1, len, len, 10, syms, (const int32_t *)dpts.p, nullptr, (const double *)dfd.p,
                                    (const ofdm_fc32 *)dhk.p, n_fft_, nullptr, (float *)dq.p), "ofdm_rx_quality_batch");
        float row[OFDM_QUALITY_FIELDS];
        check(ofdm_memcpy_d2h(ctx_, row, dq.p, sizeof(row)), "d2h");
        q.valid = row[OFDM_Q_VALID] != 0.f;
        q.noise_var = row[OFDM_Q_NOISE_VAR]; q.gain = row[OFDM_Q_GAIN]; q.llr_unit = row[OFDM_Q_LLR_UNIT]; q.points = row[OFDM_Q_POINTS];
        if (q.valid) q.snr_db = 10.0f * std::log10(row[OFDM_Q_SNR]);
        if (q.points > 0.f) q.evm_db = 10.0f * std::log10(row[OFDM_Q_EVM2]);
        return q;
    }
    // wide CFO acquisition (EXT-8, include/ofdm_hip.h; cfo_mode = OFDM_CFO_WIDE applies it inside decode with span = OFDM_CFO_WIDE_SPAN; this
    // is the bare stage): the whole multiples of 2 pi / S that the Schmidl-Cox estimate f_delta (+-pi / S, +-0.4 sub-carrier spacings) cannot
    // see, from the five training blocks of the frame that starts at sample `offset` of the capture
    struct CfoWide { int32_t m = 0; double f_delta = 0.0; float metric[2] = {0.f, 0.f}; };
    CfoWide cfo_wide(const ofdm_fc32 *fc, int64_t n, int32_t offset, double f_delta, int32_t span = OFDM_CFO_WIDE_SPAN) {
        CfoWide r;
        r.f_delta = f_delta;
        DevBuf din(ctx_, (size_t)n * sizeof(ofdm_fc32)), doff(ctx_, sizeof(int32_t)), dfd(ctx_, sizeof(double)), dm(ctx_, sizeof(int32_t)),
            dg(ctx_, 2 * sizeof(float));
        check(ofdm_memcpy_h2d(ctx_, din.p, fc, (size_t)n * sizeof(ofdm_fc32)), "h2d");
        check(ofdm_memcpy_h2d(ctx_, doff.p, &offset, sizeof(int32_t)), "h2d");
        check(ofdm_memcpy_h2d(ctx_, dfd.p, &f_delta, sizeof(double)), "h2d");
        check(ofdm_cfo_wide_batch(ctx_, (const ofdm_fc32 *)din.p, 1, n, n, (const int32_t *)doff.p, nullptr, span, (double *)dfd.p, (int32_t *)dm.p,
                                  (float *)dg.p), "ofdm_cfo_wide_batch");
        check(ofdm_memcpy_d2h(ctx_, &r.m, dm.p, sizeof(int32_t)), "d2h");
        check(ofdm_memcpy_d2h(ctx_, &r.f_delta, dfd.p, sizeof(double)), "d2h");
        check(ofdm_memcpy_d2h(ctx_, r.metric, dg.p, sizeof(r.metric)), "d2h");
        return r;
    }
    // batches on host memory: H2D / kernels / D2H pipelined inside the library (ofdm_rx_decode_host, ofdm_tx_encode_host)
    struct BatchResult { std::vector<uint8_t> bytes; int64_t row = 0; std::vector<int32_t> len, status, offset; std::vector<double> f_delta; };
    BatchResult decode_batch(const ofdm_fc32 *frames, int64_t n_frames, int64_t frame_stride, int64_t frame_len, int32_t max_symbols,
                             int64_t n_lags = 0, int64_t chunk_frames = 0) {
        BatchResult r;
        r.row = std::max<int64_t>((int64_t)max_symbols * ofdm_bytes_per_symbol(ctx_) - 16, 4);
        r.bytes.resize((size_t)(n_frames * r.row));
        r.len.resize((size_t)n_frames); r.status.resize((size_t)n_frames); r.offset.resize((size_t)n_frames); r.f_delta.resize((size_t)n_frames);
        check(ofdm_rx_decode_host(ctx_, frames, n_frames, frame_stride, frame_len, n_lags, max_symbols, r.bytes.data(), r.row, r.len.data(),
                                  r.status.data(), r.offset.data(), r.f_delta.data(), nullptr, chunk_frames), "ofdm_rx_decode_host");
        return r;
    }
    // EXT-9: the same on sc16 host samples (interleaved int16 I/Q as a radio delivers them; x = int16 * scale): half the H2D bytes
    BatchResult decode_batch_sc16(const ofdm_sc16 *frames, int64_t n_frames, int64_t frame_stride, int64_t frame_len, int32_t max_symbols,
                                  float scale = OFDM_SC16_DEFAULT_SCALE, int64_t n_lags = 0, int64_t chunk_frames = 0) {
        BatchResult r;
        r.row = std::max<int64_t>((int64_t)max_symbols * ofdm_bytes_per_symbol(ctx_) - 16, 4);
        r.bytes.resize((size_t)(n_frames * r.row));
        r.len.resize((size_t)n_frames); r.status.resize((size_t)n_frames); r.offset.resize((size_t)n_frames); r.f_delta.resize((size_t)n_frames);
        check(ofdm_rx_decode_sc16_host(ctx_, frames, n_frames, frame_stride, frame_len, scale, n_lags, max_symbols, r.bytes.data(), r.row,
                                       r.len.data(), r.status.data(), r.offset.data(), r.f_delta.data(), nullptr, chunk_frames),
              "ofdm_rx_decode_sc16_host");
        return r;
    }
    // rx_demod of regular sc16 streams on host memory -> n_frames rows of syms_per_frame * bytes_per_symbol bytes
    std::vector<uint8_t> demod_batch_sc16(const ofdm_sc16 *frames, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                                          int32_t syms_per_frame, int32_t first_symbol = 0, float scale = OFDM_SC16_DEFAULT_SCALE,
                                          int64_t chunk_frames = 0) {
        const int64_t nb = (int64_t)syms_per_frame * ofdm_bytes_per_symbol(ctx_);
        std::vector<uint8_t> out((size_t)(n_frames * nb));
        check(ofdm_rx_demod_sc16_host(ctx_, frames, n_frames, frame_stride, frame_len, scale, first_symbol, syms_per_frame, out.data(), nb,
                                      chunk_frames), "ofdm_rx_demod_sc16_host");
        return out;
    }
    // the two stages on the device (k_sc16_widen / k_sc16_narrow), host vectors in and out; *clipped (optional): clipped components
    std::vector<ofdm_fc32> sc16_widen(const std::vector<ofdm_sc16> &in, float scale = OFDM_SC16_DEFAULT_SCALE) {
        const int64_t n = (int64_t)in.size();
        DevBuf din(ctx_, in.size() * sizeof(ofdm_sc16)), dout(ctx_, in.size() * sizeof(ofdm_fc32));
        std::vector<ofdm_fc32> out(in.size());
        if (n) check(ofdm_memcpy_h2d(ctx_, din.p, in.data(), in.size() * sizeof(ofdm_sc16)), "h2d");
        check(ofdm_sc16_widen_batch(ctx_, (const ofdm_sc16 *)din.p, n ? 1 : 0, n, n, scale, (ofdm_fc32 *)dout.p, n), "ofdm_sc16_widen_batch");
        if (n) check(ofdm_memcpy_d2h(ctx_, out.data(), dout.p, out.size() * sizeof(ofdm_fc32)), "d2h");
        return out;
    }
    std::vector<ofdm_sc16> sc16_narrow(const std::vector<ofdm_fc32> &in, float scale = 1.0f / OFDM_SC16_DEFAULT_SCALE, int32_t *clipped = nullptr) {
        const int64_t n = (int64_t)in.size();
        DevBuf din(ctx_, in.size() * sizeof(ofdm_fc32)), dout(ctx_, in.size() * sizeof(ofdm_sc16)), dclip(ctx_, sizeof(int32_t));
        std::vector<ofdm_sc16> out(in.size());
        if (clipped) *clipped = 0;
        if (!n) return out;
        check(ofdm_memcpy_h2d(ctx_, din.p, in.data(), in.size() * sizeof(ofdm_fc32)), "h2d");
        check(ofdm_sc16_narrow_batch(ctx_, (const ofdm_fc32 *)din.p, 1, n, n, scale, (ofdm_sc16 *)dout.p, n, (int32_t *)dclip.p), "ofdm_sc16_narrow_batch");
        check(ofdm_memcpy_d2h(ctx_, out.data(), dout.p, out.size() * sizeof(ofdm_sc16)), "d2h");
        if (clipped) check(ofdm_memcpy_d2h(ctx_, clipped, dclip.p, sizeof(int32_t)), "d2h");
        return out;
    }
    // soft combining (EXT-7, include/ofdm_hip.h): frames of n_branches captures each, capture r of frame f at frames[(f * n_branches + r) *
    // frame_stride ..] -- two antennas, or a frame received twice -- decoded once per frame from the captures' LLRs weighted by link quality.
    // The captures are copied to the device and the results back by this call (the chain itself works on device buffers).  Modes: the
    // framed convolutional and the LDPC modes, alone or under RS / the frame check; every other mode throws (OFDM_ERR_UNSUPPORTED).
    struct CombineResult { std::vector<uint8_t> bytes; int64_t row = 0; std::vector<int32_t> len, status, branch_status, weight; };
    CombineResult decode_combine(const ofdm_fc32 *frames, int64_t n_frames, int32_t n_branches, int64_t frame_stride, int64_t frame_len,
                                 int32_t max_symbols, int64_t n_lags = 0) {
        CombineResult r;
        const size_t nf = (size_t)n_frames, rows = nf * (size_t)n_branches;
        r.row = std::max<int64_t>((int64_t)max_symbols * ofdm_bytes_per_symbol(ctx_) - 16, 4);
        if (rs_outer(base_ecc(ecc_))) r.row = ofdm_rs255_decoded_len(r.row); // whole 223-byte blocks, the trailing zero block included
        r.bytes.resize(nf * (size_t)r.row);
        r.len.resize(nf); r.status.resize(nf); r.branch_status.resize(rows); r.weight.resize(rows);
        if (!n_frames) return r;
        const size_t samples = (rows - 1) * (size_t)frame_stride + (size_t)frame_len;
        DevBuf din(ctx_, samples * sizeof(ofdm_fc32)), dout(ctx_, r.bytes.size()), dlen(ctx_, nf * 4), dst(ctx_, nf * 4), dbs(ctx_, rows * 4), dw(ctx_, rows * 4);
        check(ofdm_memcpy_h2d(ctx_, din.p, frames, samples * sizeof(ofdm_fc32)), "h2d");
        check(ofdm_rx_decode_combine_batch(ctx_, (const ofdm_fc32 *)din.p, n_frames, n_branches, frame_stride, frame_len, n_lags, max_symbols,
                                           (uint8_t *)dout.p, r.row, (int32_t *)dlen.p, (int32_t *)dst.p, (int32_t *)dbs.p, nullptr, nullptr, nullptr,
                                           (int32_t *)dw.p, nullptr), "ofdm_rx_decode_combine_batch");
        check(ofdm_memcpy_d2h(ctx_, r.bytes.data(), dout.p, r.bytes.size()), "d2h");
        check(ofdm_memcpy_d2h(ctx_, r.len.data(), dlen.p, nf * 4), "d2h");
        check(ofdm_memcpy_d2h(ctx_, r.status.data(), dst.p, nf * 4), "d2h");
        check(ofdm_memcpy_d2h(ctx_, r.branch_status.data(), dbs.p, rows * 4), "d2h");
        check(ofdm_memcpy_d2h(ctx_, r.weight.data(), dw.p, rows * 4), "d2h");
        return r;
    }
    // the stage alone on host rows: n_frames * n_branches rows of n_llr int8 LLRs -> n_frames combined rows; quality (rows of
    // OFDM_QUALITY_FIELDS floats), status and n_live (int32 per branch row) are optional
    std::vector<int8_t> llr_combine(const int8_t *llr, int64_t n_frames, int32_t n_branches, int64_t n_llr, const float *quality = nullptr,
                                    const int32_t *status = nullptr, const int32_t *n_live = nullptr) {
        const size_t rows = (size_t)n_frames * (size_t)n_branches, nl = (size_t)n_llr;
        std::vector<int8_t> out((size_t)n_frames * nl);
        if (!n_frames) return out;
        DevBuf din(ctx_, rows * nl), dout(ctx_, out.size()), dq(ctx_, rows * OFDM_QUALITY_FIELDS * sizeof(float)), dst(ctx_, rows * 4), dnl(ctx_, rows * 4);
        check(ofdm_memcpy_h2d(ctx_, din.p, llr, rows * nl), "h2d");
        if (quality) check(ofdm_memcpy_h2d(ctx_, dq.p, quality, rows * OFDM_QUALITY_FIELDS * sizeof(float)), "h2d");
        if (status) check(ofdm_memcpy_h2d(ctx_, dst.p, status, rows * 4), "h2d");
        if (n_live) check(ofdm_memcpy_h2d(ctx_, dnl.p, n_live, rows * 4), "h2d");
        check(ofdm_llr_combine_batch(ctx_, (const int8_t *)din.p, n_frames, n_branches, n_llr, n_llr, quality ? (const float *)dq.p : nullptr,
                                     status ? (const int32_t *)dst.p : nullptr, n_live ? (const int32_t *)dnl.p : nullptr, (int8_t *)dout.p, n_llr,
                                     nullptr), "ofdm_llr_combine_batch");
        check(ofdm_memcpy_d2h(ctx_, out.data(), dout.p, out.size()), "d2h");
        return out;
    }
    std::vector<ofdm_fc32> encode_batch(const uint8_t *payload, int64_t n_frames, int32_t payload_bytes, int64_t chunk_frames = 0) {
        const int64_t frame = ofdm_frame_samples(ctx_, payload_bytes);
        std::vector<ofdm_fc32> out((size_t)(n_frames * frame));
        check(ofdm_tx_encode_host(ctx_, payload, n_frames, payload_bytes, nullptr, payload_bytes, out.data(), frame, chunk_frames),
              "ofdm_tx_encode_host");
        return out;
    }
    // modulate / demodulate (src/transmitter.rs:108-140, src/receiver.rs:147-190)
    std::vector<Complex64> modulate(const std::vector<uint8_t> &stream) {
        ofdm_params q; (void)q;
        const int bps = 8 * ofdm_bytes_per_symbol(ctx_) / ofdm_data_carriers(ctx_);
        const size_t n = (stream.size() * 8 + bps - 1) / bps;
        DevBuf din(ctx_, stream.size()), dout(ctx_, n * sizeof(ofdm_fc32));
        check(ofdm_memcpy_h2d(ctx_, din.p, stream.data(), stream.size()), "h2d");
        check(ofdm_qam_map_batch(ctx_, (const uint8_t *)din.p, (int64_t)stream.size(), (ofdm_fc32 *)dout.p), "ofdm_qam_map_batch");
        std::vector<ofdm_fc32> host(n);
        check(ofdm_memcpy_d2h(ctx_, host.data(), dout.p, n * sizeof(ofdm_fc32)), "d2h");
        return from_fc32(host);
    }
    std::vector<uint8_t> demodulate(const std::vector<Complex64> &stream) {
        const auto fc = to_fc32(stream);
        const int bps = 8 * ofdm_bytes_per_symbol(ctx_) / ofdm_data_carriers(ctx_);
        std::vector<uint8_t> out(fc.size() * bps / 8);
        DevBuf din(ctx_, fc.size() * sizeof(ofdm_fc32)), dout(ctx_, out.size());
        check(ofdm_memcpy_h2d(ctx_, din.p, fc.data(), fc.size() * sizeof(ofdm_fc32)), "h2d");
        check(ofdm_qam_demap_batch(ctx_, (const ofdm_fc32 *)din.p, (int64_t)fc.size(), (uint8_t *)dout.p, nullptr),
              "ofdm_qam_demap_batch"); // OFDM_ERR_INVALID unless size % 8 == 0 (assert at src/receiver.rs:153)
        if (!out.empty()) check(ofdm_memcpy_d2h(ctx_, out.data(), dout.p, out.size()), "d2h");
        return out;
    }
    // K = 7 rate-1/2 convolutional code (OFDM_ECC_CONV_K7 as the context's ecc applies it inside encode / decode; these are the bare
    // stages): payload -> 2 (n + 1) coded bytes, and 2 n_steps int8 LLRs (positive = bit 1) -> n_steps / 8 bytes by Viterbi decoding
    std::vector<uint8_t> conv_encode(const std::vector<uint8_t> &data) {
        std::vector<uint8_t> out(2 * (data.size() + 1));
        DevBuf din(ctx_, data.size()), dout(ctx_, out.size());
        if (!data.empty()) check(ofdm_memcpy_h2d(ctx_, din.p, data.data(), data.size()), "h2d");
        check(ofdm_conv_k7_encode(ctx_, (const uint8_t *)din.p, 1, (int64_t)data.size(), (int64_t)data.size(), (uint8_t *)dout.p,
                                  (int64_t)out.size()), "ofdm_conv_k7_encode");
        check(ofdm_memcpy_d2h(ctx_, out.data(), dout.p, out.size()), "d2h");
        return out;
    }
    std::vector<uint8_t> viterbi_decode_soft(const std::vector<int8_t> &llr, bool terminated = true) {
        const int64_t n_steps = (int64_t)(llr.size() / 2);
        std::vector<uint8_t> out((size_t)(n_steps / 8));
        DevBuf din(ctx_, llr.size()), dout(ctx_, out.size());
        if (!llr.empty()) check(ofdm_memcpy_h2d(ctx_, din.p, llr.data(), llr.size()), "h2d");
        check(ofdm_conv_k7_decode_soft(ctx_, (const int8_t *)din.p, 1, 2 * n_steps, n_steps, terminated ? 1 : 0, (uint8_t *)dout.p,
                                       (int64_t)out.size()), "ofdm_conv_k7_decode_soft");
        if (!out.empty()) check(ofdm_memcpy_d2h(ctx_, out.data(), dout.p, out.size()), "d2h");
        return out;
    }
    // the same pair at a punctured rate (OFDM_CONV_RATE_1_2 / _2_3 / _3_4; the framed modes OFDM_ECC_CONV_K7F_* apply it inside encode /
    // decode): payload -> ceil(kept(8 (n + 1), rate) / 8) bytes, and the kept(n_steps, rate) LLRs of n_steps steps -> n_steps / 8 bytes
    static int64_t conv_kept_bits(int64_t n_steps, int rate) { return ofdm_conv_k7_kept_bits(n_steps, rate); }
    std::vector<uint8_t> conv_encode_punctured(const std::vector<uint8_t> &data, int rate) {
        const int64_t kept = ofdm_conv_k7_kept_bits(8 * ((int64_t)data.size() + 1), rate);
        check(kept < 0 ? (int)kept : 0, "ofdm_conv_k7_kept_bits");
        std::vector<uint8_t> out((size_t)((kept + 7) / 8));
        DevBuf din(ctx_, data.size()), dout(ctx_, out.size());
        if (!data.empty()) check(ofdm_memcpy_h2d(ctx_, din.p, data.data(), data.size()), "h2d");
        check(ofdm_conv_k7_encode_punctured(ctx_, (const uint8_t *)din.p, 1, (int64_t)data.size(), (int64_t)data.size(), rate,
                                            (uint8_t *)dout.p, (int64_t)out.size()), "ofdm_conv_k7_encode_punctured");
        check(ofdm_memcpy_d2h(ctx_, out.data(), dout.p, out.size()), "d2h");
        return out;
    }
    std::vector<uint8_t> viterbi_decode_punctured(const std::vector<int8_t> &llr, int64_t n_steps, int rate, bool terminated = true) {
        std::vector<uint8_t> out((size_t)(n_steps > 0 ? n_steps / 8 : 0));
        DevBuf din(ctx_, llr.size()), dout(ctx_, out.size());
        if (!llr.empty()) check(ofdm_memcpy_h2d(ctx_, din.p, llr.data(), llr.size()), "h2d");
        check(ofdm_conv_k7_decode_punctured(ctx_, (const int8_t *)din.p, 1, (int64_t)llr.size(), n_steps, rate, terminated ? 1 : 0,
                                            (uint8_t *)dout.p, (int64_t)out.size()), "ofdm_conv_k7_decode_punctured");
        if (!out.empty()) check(ofdm_memcpy_d2h(ctx_, out.data(), dout.p, out.size()), "d2h");
        return out;
    }
    // outer Reed-Solomon(255,223) on the device (the OFDM_ECC_RS255* modes apply it inside encode / decode): one row ->
    // 255 (n / 223 + 1) code bytes, and one row of code bytes -> 223 (n / 255 + 1) bytes; *corrected = corrected bytes, -1 if a
    // block has more than 16 errors (its data bytes come back as received)
    std::vector<uint8_t> rs255_encode(const std::vector<uint8_t> &data) {
        std::vector<uint8_t> out((size_t)ofdm_rs255_encoded_len((int64_t)data.size()));
        DevBuf din(ctx_, data.size()), dout(ctx_, out.size());
        if (!data.empty()) check(ofdm_memcpy_h2d(ctx_, din.p, data.data(), data.size()), "h2d");
        check(ofdm_rs255_encode_batch(ctx_, (const uint8_t *)din.p, 1, (int64_t)data.size(), nullptr, (int64_t)data.size(), (uint8_t *)dout.p,
                                      (int64_t)out.size()), "ofdm_rs255_encode_batch");
        check(ofdm_memcpy_d2h(ctx_, out.data(), dout.p, out.size()), "d2h");
        return out;
    }
    std::vector<uint8_t> rs255_decode(const std::vector<uint8_t> &code, int32_t *corrected = nullptr) {
        std::vector<uint8_t> out((size_t)ofdm_rs255_decoded_len((int64_t)code.size()));
        DevBuf din(ctx_, code.size()), dout(ctx_, out.size()), dfix(ctx_, sizeof(int32_t));
        if (!code.empty()) check(ofdm_memcpy_h2d(ctx_, din.p, code.data(), code.size()), "h2d");
        check(ofdm_rs255_decode_batch(ctx_, (const uint8_t *)din.p, 1, (int64_t)code.size(), nullptr, (int64_t)code.size(), (uint8_t *)dout.p,
                                      (int64_t)out.size(), nullptr, (int32_t *)dfix.p), "ofdm_rs255_decode_batch");
        check(ofdm_memcpy_d2h(ctx_, out.data(), dout.p, out.size()), "d2h");
        if (corrected) check(ofdm_memcpy_d2h(ctx_, corrected, dfix.p, sizeof(int32_t)), "d2h");
        return out;
    }
    // LDPC(648,324) on the device (OFDM_ECC_LDPC648 applies it inside encode / decode; these are the bare stages): whole 40-byte blocks ->
    // 80 code bytes each, and whole code words of 640 LLRs (positive = bit 1) -> 40 bytes each; iters (optional): per code word the
    // iteration it converged at, 0 if it did not within max_iter
    std::vector<uint8_t> ldpc_encode(const std::vector<uint8_t> &info) {
        if (info.size() % 40) throw Error("ldpc_encode: whole 40-byte blocks expected");
        std::vector<uint8_t> out(2 * info.size());
        DevBuf din(ctx_, info.size()), dout(ctx_, out.size());
        if (!info.empty()) check(ofdm_memcpy_h2d(ctx_, din.p, info.data(), info.size()), "h2d");
        check(ofdm_ldpc648_encode_batch(ctx_, (const uint8_t *)din.p, 1, (int64_t)info.size(), (int64_t)(info.size() / 40), (uint8_t *)dout.p,
                                        (int64_t)out.size()), "ofdm_ldpc648_encode_batch");
        if (!out.empty()) check(ofdm_memcpy_d2h(ctx_, out.data(), dout.p, out.size()), "d2h");
        return out;
    }
    std::vector<uint8_t> ldpc_decode(const std::vector<int8_t> &llr, int32_t max_iter = OFDM_LDPC_MAX_ITER, std::vector<int32_t> *iters = nullptr) {
        if (llr.size() % 640) throw Error("ldpc_decode: whole code words of 640 LLRs expected");
        const size_t n_cw = llr.size() / 640;
        std::vector<uint8_t> out(40 * n_cw);
        DevBuf din(ctx_, llr.size()), dout(ctx_, out.size()), dit(ctx_, sizeof(int32_t) * n_cw);
        if (!llr.empty()) check(ofdm_memcpy_h2d(ctx_, din.p, llr.data(), llr.size()), "h2d");
        check(ofdm_ldpc648_decode_batch(ctx_, (const int8_t *)din.p, 1, (int64_t)llr.size(), (int64_t)n_cw, max_iter, (uint8_t *)dout.p,
                                        (int64_t)out.size(), (int32_t *)dit.p), "ofdm_ldpc648_decode_batch");
        if (!out.empty()) check(ofdm_memcpy_d2h(ctx_, out.data(), dout.p, out.size()), "d2h");
        if (iters) { iters->resize(n_cw); if (n_cw) check(ofdm_memcpy_d2h(ctx_, iters->data(), dit.p, sizeof(int32_t) * n_cw), "d2h"); }
        return out;
    }
    // ... and over the family: rate 0 = 1/2 (the two above), 1 = 2/3, 2 = 3/4, 3 = 5/6; K = ofdm_ldpc648_info_bytes(rate) info bytes a code word
    std::vector<uint8_t> ldpc_encode(const std::vector<uint8_t> &info, int32_t rate) {
        const int32_t k = ofdm_ldpc648_info_bytes(rate);
        if (k <= 0) throw Error("ldpc_encode: rate must be 0 .. 3");
        if (info.size() % (size_t)k) throw Error("ldpc_encode: whole blocks of K info bytes expected");
        const size_t n_cw = info.size() / (size_t)k;
        std::vector<uint8_t> out(80 * n_cw);
        DevBuf din(ctx_, info.size()), dout(ctx_, out.size());
        if (!info.empty()) check(ofdm_memcpy_h2d(ctx_, din.p, info.data(), info.size()), "h2d");
        check(ofdm_ldpc648_encode_rate_batch(ctx_, (const uint8_t *)din.p, 1, (int64_t)info.size(), (int64_t)n_cw, rate, (uint8_t *)dout.p,
                                             (int64_t)out.size()), "ofdm_ldpc648_encode_rate_batch");
        if (!out.empty()) check(ofdm_memcpy_d2h(ctx_, out.data(), dout.p, out.size()), "d2h");
        return out;
    }
    std::vector<uint8_t> ldpc_decode(const std::vector<int8_t> &llr, int32_t max_iter, int32_t rate, std::vector<int32_t> *iters = nullptr) {
        const int32_t k = ofdm_ldpc648_info_bytes(rate);
        if (k <= 0) throw Error("ldpc_decode: rate must be 0 .. 3");
        if (llr.size() % 640) throw Error("ldpc_decode: whole code words of 640 LLRs expected");
        const size_t n_cw = llr.size() / 640;
        std::vector<uint8_t> out((size_t)k * n_cw);
        DevBuf din(ctx_, llr.size()), dout(ctx_, out.size()), dit(ctx_, sizeof(int32_t) * n_cw);
        if (!llr.empty()) check(ofdm_memcpy_h2d(ctx_, din.p, llr.data(), llr.size()), "h2d");
        check(ofdm_ldpc648_decode_rate_batch(ctx_, (const int8_t *)din.p, 1, (int64_t)llr.size(), (int64_t)n_cw, max_iter, rate, (uint8_t *)dout.p,
                                             (int64_t)out.size(), (int32_t *)dit.p), "ofdm_ldpc648_decode_rate_batch");
        if (!out.empty()) check(ofdm_memcpy_d2h(ctx_, out.data(), dout.p, out.size()), "d2h");
        if (iters) { iters->resize(n_cw); if (n_cw) check(ofdm_memcpy_d2h(ctx_, iters->data(), dit.p, sizeof(int32_t) * n_cw), "d2h"); }
        return out;
    }
    // CRC-32 frame check on the device (the OFDM_ECC_FCS + mode contexts apply it inside encode / decode; these are the bare stages):
    // one row -> its envelope [u32 LE n][data][u32 LE crc32 of both], and one delivered row -> the payload of a valid envelope, or
    // nullopt (bytes behind the envelope are ignored)
    std::vector<uint8_t> fcs_wrap(const std::vector<uint8_t> &data) {
        std::vector<uint8_t> out(data.size() + OFDM_FCS_OVERHEAD);
        DevBuf din(ctx_, data.size()), dout(ctx_, out.size());
        if (!data.empty()) check(ofdm_memcpy_h2d(ctx_, din.p, data.data(), data.size()), "h2d");
        check(ofdm_fcs_wrap_batch(ctx_, (const uint8_t *)din.p, 1, (int64_t)data.size(), nullptr, (int64_t)data.size(), (uint8_t *)dout.p,
                                  (int64_t)out.size(), nullptr), "ofdm_fcs_wrap_batch");
        check(ofdm_memcpy_d2h(ctx_, out.data(), dout.p, out.size()), "d2h");
        return out;
    }
    std::optional<std::vector<uint8_t>> fcs_check(const std::vector<uint8_t> &row) {
        std::vector<uint8_t> out(row.size() > OFDM_FCS_OVERHEAD ? row.size() - OFDM_FCS_OVERHEAD : 0);
        DevBuf din(ctx_, row.size()), dout(ctx_, out.size()), dres(ctx_, 2 * sizeof(int32_t));
        if (!row.empty()) check(ofdm_memcpy_h2d(ctx_, din.p, row.data(), row.size()), "h2d");
        check(ofdm_fcs_check_batch(ctx_, (const uint8_t *)din.p, 1, (int64_t)row.size(), nullptr, (int64_t)row.size(), (uint8_t *)dout.p,
                                   (int64_t)out.size(), (int32_t *)dres.p, (int32_t *)dres.p + 1), "ofdm_fcs_check_batch");
        int32_t res[2] = {0, 0}; // out_len, ok
        check(ofdm_memcpy_d2h(ctx_, res, dres.p, sizeof(res)), "d2h");
        if (!res[1]) return std::nullopt;
        if (!out.empty()) check(ofdm_memcpy_d2h(ctx_, out.data(), dout.p, out.size()), "d2h");
        out.resize((size_t)res[0]);
        return out;
    }
    // channel-estimate denoising (EXT-5; OFDM_CHEST_WLS as the context's chest_mode applies it inside decode; this is the bare stage):
    // rows of n_fft bins of an estimate -> the weighted least-squares fit of cp_len taps to every row, as n_fft bins again
    std::vector<Complex64> chest_smooth(const std::vector<Complex64> &hk) {
        const auto fc = to_fc32(hk);
        std::vector<ofdm_fc32> host(fc.size());
        DevBuf d(ctx_, fc.size() * sizeof(ofdm_fc32));
        if (!fc.empty()) check(ofdm_memcpy_h2d(ctx_, d.p, fc.data(), fc.size() * sizeof(ofdm_fc32)), "h2d");
        check(ofdm_chest_smooth_batch(ctx_, (const ofdm_fc32 *)d.p, (int64_t)fc.size() / n_fft_, (ofdm_fc32 *)d.p), "ofdm_chest_smooth_batch");
        if (!fc.empty()) check(ofdm_memcpy_d2h(ctx_, host.data(), d.p, host.size() * sizeof(ofdm_fc32)), "d2h");
        return from_fc32(host);
    }
    // (first_tap, n_taps) = (-cp_len / 4, cp_len): the delays the denoised estimate may occupy
    std::pair<int32_t, int32_t> chest_window() const {
        int32_t first = 0, n = 0;
        check(ofdm_chest_window(ctx_, &first, &n), "ofdm_chest_window");
        return {first, n};
    }
    // R^-1 of the stage's normal equations for the default training table, cp_len x cp_len, row-major (host call, f64)
    static std::vector<Complex64> chest_matrix(int n_fft) {
        std::vector<double> r(2 * (size_t)(n_fft / 4) * (size_t)(n_fft / 4));
        check(ofdm_chest_matrix(n_fft, n_fft / 4, nullptr, r.data()), "ofdm_chest_matrix");
        std::vector<Complex64> o(r.size() / 2);
        for (size_t i = 0; i < o.size(); ++i) o[i] = Complex64(r[2 * i], r[2 * i + 1]);
        return o;
    }

  private:
    // is `ecc` one of the modes with the outer Reed-Solomon code around the inner mode's frame (20 + inner)?
    static bool rs_outer(int ecc) {
        return ecc == OFDM_ECC_RS255 || ecc == OFDM_ECC_RS255_K7F_R12 || ecc == OFDM_ECC_RS255_K7F_R23 ||
               ecc == OFDM_ECC_RS255_K7F_R34;
    }
    // the mode under the frame check of an OFDM_ECC_FCS + mode value, else ecc itself
    static int base_ecc(int ecc) { return ecc >= OFDM_ECC_FCS ? ecc - OFDM_ECC_FCS : ecc; }
    ofdm_ctx *ctx_ = nullptr;
    int ecc_ = OFDM_ECC_NONE;
    int n_fft_ = 64;
    int window_reps_ = 3;
};

// EXT-14: a streaming receiver on a context (ofdm_stream_create .. ofdm_stream_state, include/ofdm_hip.h "a streaming receiver").  push()
// takes the samples as a radio hands them over and returns the packets this push made deliverable -- however the stream is cut, they are,
// bit for bit, the packets of one ofdm_rx_decode_all_long_host call on the concatenation, each exactly once.  Destroy it before its context.
class Stream {
  public:
    struct Packet { std::vector<uint8_t> bytes; int32_t status = 0; int64_t offset = 0, d1 = 0, d_hat = 0; double f_delta = 0.0; float metric = 0.f; };
    struct State { int64_t total = 0, kept_from = 0, next_lag = 0; bool ended = false; };
    Stream(Context &ctx, int32_t max_symbols, int64_t holdoff = 0, int64_t max_chunk = 65536, int64_t first_sample = 0) {
        check(ofdm_stream_create(&s_, ctx.raw(), max_symbols, holdoff > 0 ? holdoff : ctx.default_holdoff(), max_chunk, first_sample),
              "ofdm_stream_create");
        // at least the decode row size of every mode (the RS modes deliver whole 223-byte blocks, the trailing zero block included)
        row_ = std::max<int64_t>((int64_t)max_symbols * ofdm_bytes_per_symbol(ctx.raw()), 4) + 256;
    }
    ~Stream() { if (s_) ofdm_stream_destroy(s_); }
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    std::vector<Packet> push(const ofdm_fc32 *fc, int64_t n, bool flush = false) {
        return drained([&](Out &o, bool first) {
            return ofdm_stream_push(s_, first ? fc : nullptr, first ? n : 0, flush, kBatch, o.rows.data(), row_, o.len, o.status, o.offset, o.f_delta,
                                    o.metric, o.d1, o.d_hat, &o.n, &o.more);
        });
    }
    std::vector<Packet> push_sc16(const ofdm_sc16 *sc, int64_t n, float scale = OFDM_SC16_DEFAULT_SCALE, bool flush = false) {
        return drained([&](Out &o, bool first) {
            return first ? ofdm_stream_push_sc16(s_, sc, n, scale, flush, kBatch, o.rows.data(), row_, o.len, o.status, o.offset, o.f_delta, o.metric,
                                                 o.d1, o.d_hat, &o.n, &o.more)
                         : ofdm_stream_push(s_, nullptr, 0, flush, kBatch, o.rows.data(), row_, o.len, o.status, o.offset, o.f_delta, o.metric, o.d1,
                                            o.d_hat, &o.n, &o.more);
        });
    }
    // every remaining detection, a last frame cut by the end of the stream included; the stream is ended until reset()
    std::vector<Packet> flush() { return push(nullptr, 0, true); }
    void reset(int64_t first_sample = 0) { check(ofdm_stream_reset(s_, first_sample), "ofdm_stream_reset"); }
    // EXT-15: the DC blocker in front of the window (0 = off; DcBlock::default_blocks for the usual window).  Only before the first sample
    // or right after reset(), which keeps the setting and clears the filter's history
    void set_dc_block(int32_t blocks) { check(ofdm_stream_set_dc_block(s_, blocks), "ofdm_stream_set_dc_block"); }
    int32_t dc_block() const {
        int32_t m = 0;
        check(ofdm_stream_get_dc_block(s_, &m), "ofdm_stream_get_dc_block");
        return m;
    }
    // EXT-16: the down-converter in front of everything else (decim 0 = off; taps empty: the default design).  Pushes are then
    // input-rate samples; holdoff, first_sample and every offset are in OUTPUT samples.  Only before the first sample or right after
    // reset(), which keeps the setting and clears the history
    void set_ddc(int32_t decim, int32_t phase_inc = 0, const std::vector<float> &taps = {}) {
        check(ofdm_stream_set_ddc(s_, decim, phase_inc, taps.empty() ? nullptr : taps.data(), (int32_t)taps.size()), "ofdm_stream_set_ddc");
    }
    struct DdcSetting { int32_t decim = 0, phase_inc = 0, n_taps = 0; };
    DdcSetting ddc() const {
        DdcSetting d;
        check(ofdm_stream_get_ddc(s_, &d.decim, &d.phase_inc, &d.n_taps), "ofdm_stream_get_ddc");
        return d;
    }
    State state() const {
        State st; int32_t ended = 0;
        check(ofdm_stream_state(s_, &st.total, &st.kept_from, &st.next_lag, &ended), "ofdm_stream_state");
        st.ended = ended != 0;
        return st;
    }

  private:
    static constexpr int64_t kBatch = 64; // packets taken per call; the rest is drained through `more`
    struct Out {
        std::vector<uint8_t> rows; int32_t len[kBatch], status[kBatch], more = 0; int64_t offset[kBatch], d1[kBatch], d_hat[kBatch], n = 0;
        double f_delta[kBatch]; float metric[kBatch];
    };
    template <class Call> std::vector<Packet> drained(Call &&call) {
        std::vector<Packet> out;
        Out o;
        o.rows.resize((size_t)(kBatch * row_));
        bool first = true;
        do {
            check(call(o, first), "ofdm_stream_push");
            first = false;
            for (int64_t k = 0; k < o.n; ++k) {
                Packet p;
                p.status = o.status[k]; p.offset = o.offset[k]; p.d1 = o.d1[k]; p.d_hat = o.d_hat[k]; p.f_delta = o.f_delta[k]; p.metric = o.metric[k];
                if (p.status == OFDM_FRAME_OK && o.len[k] > 0) p.bytes.assign(o.rows.begin() + k * row_, o.rows.begin() + k * row_ + o.len[k]);
                out.push_back(std::move(p));
            }
        } while (o.more);
        return out;
    }
    ofdm_stream *s_ = nullptr;
    int64_t row_ = 4;
};

// EXT-15: a DC blocker on device buffers (ofdm_dcblock_create .. ofdm_dcblock_state, include/ofdm_hip.h "a DC blocker in front of
// detection").  Every sample leaves less the mean of the `blocks` complete 64-sample blocks in front of its own block; the pushes of one
// filter, concatenated, equal ofdm_dc_block of the concatenated inputs bit for bit.  in_dev and out_dev are device buffers that do not
// overlap; the launches are enqueued on the context's stream.  Destroy it before its context.
class DcBlock {
  public:
    struct State { int64_t total = 0; int32_t blocks = 0; };
    static int32_t default_blocks(int32_t n_fft) {
        const int m = ofdm_dc_block_default(n_fft, n_fft / 4);
        check(m < 0 ? m : OFDM_OK, "ofdm_dc_block_default");
        return m;
    }
    DcBlock(Context &ctx, int32_t blocks, int64_t max_chunk = 1 << 20) { check(ofdm_dcblock_create(&f_, ctx.raw(), blocks, max_chunk), "ofdm_dcblock_create"); }
    ~DcBlock() { if (f_) ofdm_dcblock_destroy(f_); }
    DcBlock(const DcBlock &) = delete;
    DcBlock &operator=(const DcBlock &) = delete;
    void push(const ofdm_fc32 *in_dev, int64_t n, ofdm_fc32 *out_dev) { check(ofdm_dcblock_push(f_, in_dev, n, out_dev), "ofdm_dcblock_push"); }
    void push_sc16(const ofdm_sc16 *in_dev, int64_t n, ofdm_fc32 *out_dev, float scale = OFDM_SC16_DEFAULT_SCALE) {
        check(ofdm_dcblock_push_sc16(f_, in_dev, n, scale, out_dev), "ofdm_dcblock_push_sc16");
    }
    void reset() { check(ofdm_dcblock_reset(f_), "ofdm_dcblock_reset"); }
    State state() const {
        State st;
        check(ofdm_dcblock_state(f_, &st.total, &st.blocks), "ofdm_dcblock_state");
        return st;
    }
    // the definition on host arrays, no GPU
    static std::vector<ofdm_fc32> host(const ofdm_fc32 *in, int64_t n, int32_t blocks) {
        std::vector<ofdm_fc32> out((size_t)n);
        check(ofdm_dc_block(in, n, blocks, out.data()), "ofdm_dc_block");
        return out;
    }
    static std::vector<ofdm_fc32> host_sc16(const ofdm_sc16 *in, int64_t n, int32_t blocks, float scale = OFDM_SC16_DEFAULT_SCALE) {
        std::vector<ofdm_fc32> out((size_t)n);
        check(ofdm_dc_block_sc16(in, n, scale, blocks, out.data()), "ofdm_dc_block_sc16");
        return out;
    }

  private:
    ofdm_dcblock *f_ = nullptr;
};

// EXT-16: a digital down-converter on device buffers (ofdm_ddc_create .. ofdm_ddc_state, include/ofdm_hip.h "a digital
// down-converter"): mix by the two-level 20-bit rotor, filter by real taps, keep every decim-th sample.  The outputs of one converter's
// pushes, concatenated, equal ofdm_ddc of the concatenated inputs bit for bit.  in_dev and out_dev are device buffers that do not overlap;
// the launches are enqueued on the context's stream.  Destroy it before its context.
class Ddc {
  public:
    struct State { int64_t total_in = 0, total_out = 0; };
    // the Hamming-windowed sinc of taps_per_phase * decim taps, cutoff 0.5 / decim
    static std::vector<float> design(int32_t decim, int32_t taps_per_phase = OFDM_DDC_TAPS_PER_PHASE) {
        std::vector<float> h(decim > 0 && taps_per_phase > 0 ? (size_t)decim * (size_t)taps_per_phase : 1);
        check(ofdm_ddc_design(decim, taps_per_phase, h.data()), "ofdm_ddc_design");
        return h;
    }
    // the increment that brings f0 (cycles per input sample) to 0
    static int32_t inc_for(double f0) {
        int32_t inc = 0;
        check(ofdm_ddc_inc_for(f0, &inc), "ofdm_ddc_inc_for");
        return inc;
    }
    static int64_t out_len(int64_t n, int32_t decim, int32_t n_taps) {
        const int64_t m = ofdm_ddc_out_len(n, decim, n_taps);
        check(m < 0 ? (int)m : OFDM_OK, "ofdm_ddc_out_len");
        return m;
    }
    // the rotor tables the host definition uses and the device is given: 1024 (re, im) pairs each
    static void rotor_tables(std::vector<float> &coarse, std::vector<float> &fine) {
        coarse.resize(2048); fine.resize(2048);
        check(ofdm_ddc_rotor_tables(coarse.data(), fine.data()), "ofdm_ddc_rotor_tables");
    }
    Ddc(Context &ctx, int32_t decim, int32_t phase_inc, const std::vector<float> &taps, int64_t max_chunk = 1 << 20) {
        check(ofdm_ddc_create(&f_, ctx.raw(), decim, phase_inc, taps.data(), (int32_t)taps.size(), max_chunk), "ofdm_ddc_create");
    }
    ~Ddc() { if (f_) ofdm_ddc_destroy(f_); }
    Ddc(const Ddc &) = delete;
    Ddc &operator=(const Ddc &) = delete;
    // -> the samples written at out_dev (out_cap: what it holds)
    int64_t push(const ofdm_fc32 *in_dev, int64_t n, ofdm_fc32 *out_dev, int64_t out_cap) {
        int64_t k = 0;
        check(ofdm_ddc_push(f_, in_dev, n, out_dev, out_cap, &k), "ofdm_ddc_push");
        return k;
    }
    int64_t push_sc16(const ofdm_sc16 *in_dev, int64_t n, ofdm_fc32 *out_dev, int64_t out_cap, float scale = OFDM_SC16_DEFAULT_SCALE) {
        int64_t k = 0;
        check(ofdm_ddc_push_sc16(f_, in_dev, n, scale, out_dev, out_cap, &k), "ofdm_ddc_push_sc16");
        return k;
    }
    void reset() { check(ofdm_ddc_reset(f_), "ofdm_ddc_reset"); }
    State state() const {
        State st;
        check(ofdm_ddc_state(f_, &st.total_in, &st.total_out), "ofdm_ddc_state");
        return st;
    }
    // the definition on host arrays, no GPU
    static std::vector<ofdm_fc32> host(const ofdm_fc32 *in, int64_t n, int32_t decim, int32_t phase_inc, const std::vector<float> &taps) {
        std::vector<ofdm_fc32> out((size_t)out_len(n, decim, (int32_t)taps.size()));
        int64_t k = 0;
        check(ofdm_ddc(in, n, decim, phase_inc, taps.data(), (int32_t)taps.size(), out.data(), (int64_t)out.size(), &k), "ofdm_ddc");
        return out;
    }
    static std::vector<ofdm_fc32> host_sc16(const ofdm_sc16 *in, int64_t n, int32_t decim, int32_t phase_inc, const std::vector<float> &taps,
                                            float scale = OFDM_SC16_DEFAULT_SCALE) {
        std::vector<ofdm_fc32> out((size_t)out_len(n, decim, (int32_t)taps.size()));
        int64_t k = 0;
        check(ofdm_ddc_sc16(in, n, scale, decim, phase_inc, taps.data(), (int32_t)taps.size(), out.data(), (int64_t)out.size(), &k), "ofdm_ddc_sc16");
        return out;
    }

  private:
    ofdm_ddc_handle *f_ = nullptr;
};

// One context per (thread, parameter set), created on first use and kept: the reference's free functions are called once per
// frame (examples/lab3a.rs:24,34, jetson_rx.rs:86), and ofdm_create -- table uploads, stream and workspace set-up -- must not be
// paid on every call.  The cache is thread_local: its contexts are destroyed (ofdm_destroy: HIP calls) when the THREAD exits.  A host
// that ends threads after the HIP runtime has been torn down (static destruction order, exit() from another thread) must call
// clear_cached_contexts() on that thread first.
namespace detail {
using ContextKey = std::tuple<bool, int, int, int, int, int, int>;
inline std::map<ContextKey, std::unique_ptr<Context>> &context_cache() {
    thread_local std::map<ContextKey, std::unique_ptr<Context>> cache;
    return cache;
}
} // namespace detail
inline void clear_cached_contexts() { detail::context_cache().clear(); } // this thread's contexts, now
inline Context &cached_context(bool guard_bands, ModulationScheme m, int n_fft = 64, int ecc = OFDM_ECC_NONE,
                               int cfo_mode = OFDM_CFO_SIGNED, int device = 0) {
    using Key = detail::ContextKey;
    auto &cache = detail::context_cache();
    const Key k{guard_bands, (int)m, n_fft, ecc, cfo_mode, device, (int)default_pilot_choice()};
    auto it = cache.find(k);
    if (it == cache.end()) it = cache.emplace(k, std::make_unique<Context>(guard_bands, m, n_fft, ecc, cfo_mode, device)).first;
    return *it->second;
}

// free functions with the reference's optional-argument defaults (src/transmitter.rs:16-17, src/receiver.rs:16,83)
// fcs: the CRC-32 frame check around the payload (ecc = OFDM_ECC_FCS + OFDM_ECC_NONE): decode returns exactly the bytes that were
// sent or throws
inline std::vector<Complex64> encode(const std::vector<uint8_t> &data, std::optional<bool> guard_bands = std::nullopt,
                                     std::optional<ModulationScheme> modulation = std::nullopt, bool fcs = false) {
    return cached_context(guard_bands.value_or(false), modulation.value_or(ModulationScheme::Bpsk), 64, fcs ? OFDM_ECC_FCS : OFDM_ECC_NONE)
        .encode(data);
}
inline std::vector<uint8_t> decode(std::vector<Complex64> samples, std::optional<bool> guard_bands = std::nullopt,
                                   std::optional<ModulationScheme> modulation = std::nullopt, bool fcs = false) {
    return cached_context(guard_bands.value_or(false), modulation.value_or(ModulationScheme::Bpsk), 64, fcs ? OFDM_ECC_FCS : OFDM_ECC_NONE,
                          OFDM_CFO_ABS)
        .decode(std::move(samples));
}

// Frame-index data parallelism inside ONE process ("one host thread + one stream per device"): a context per
// entry of `devices` (an ordinal may repeat: several contexts, each with its own stream, on one GPU), a std::thread per context
// for the duration of a call, frames [r F / R, (r + 1) F / R) to context r, results written straight into the caller's arrays --
// no exchange between the devices.  The Python twin is ofdm_amd/dist.py (one process per GPU).
class ShardedContext {
  public:
    explicit ShardedContext(std::vector<int> devices, bool guard_bands = false, ModulationScheme m = ModulationScheme::Bpsk, int n_fft = 64,
                            int ecc = OFDM_ECC_NONE, int cfo_mode = OFDM_CFO_SIGNED) {
        if (devices.empty()) throw Error("ShardedContext: no device");
        for (int d : devices) {
            ctx_.push_back(std::make_unique<Context>(guard_bands, m, n_fft, ecc, cfo_mode, d));
            check(ofdm_use_own_stream(ctx_.back()->raw()), "ofdm_use_own_stream");
        }
    }
    static std::vector<int> all_devices() { // one context per visible GPU
        int n = 0;
        check(ofdm_device_count(&n), "ofdm_device_count");
        std::vector<int> d((size_t)n);
        for (int i = 0; i < n; ++i) d[(size_t)i] = i;
        return d;
    }
    size_t size() const { return ctx_.size(); }
    Context &operator[](size_t r) { return *ctx_[r]; }
    static std::pair<int64_t, int64_t> shard_range(int64_t n, int64_t r, int64_t world) { return {n * r / world, n * (r + 1) / world}; }

    Context::BatchResult decode_batch(const ofdm_fc32 *frames, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                                      int32_t max_symbols, int64_t n_lags = 0, int64_t chunk_frames = 0) {
        Context::BatchResult r;
        r.row = std::max<int64_t>((int64_t)max_symbols * ofdm_bytes_per_symbol(ctx_[0]->raw()) - 16, 4);
        r.bytes.resize((size_t)(n_frames * r.row));
        r.len.resize((size_t)n_frames); r.status.resize((size_t)n_frames); r.offset.resize((size_t)n_frames); r.f_delta.resize((size_t)n_frames);
        run([&](size_t i, int64_t lo, int64_t hi) {
            return ofdm_rx_decode_host(ctx_[i]->raw(), frames + lo * frame_stride, hi - lo, frame_stride, frame_len, n_lags, max_symbols,
                                       r.bytes.data() + lo * r.row, r.row, r.len.data() + lo, r.status.data() + lo, r.offset.data() + lo,
                                       r.f_delta.data() + lo, nullptr, chunk_frames);
        }, n_frames, "ofdm_rx_decode_host");
        return r;
    }
    std::vector<ofdm_fc32> encode_batch(const uint8_t *payload, int64_t n_frames, int32_t payload_bytes, int64_t chunk_frames = 0) {
        const int64_t frame = ofdm_frame_samples(ctx_[0]->raw(), payload_bytes);
        std::vector<ofdm_fc32> out((size_t)(n_frames * frame));
        run([&](size_t i, int64_t lo, int64_t hi) {
            return ofdm_tx_encode_host(ctx_[i]->raw(), payload + lo * payload_bytes, hi - lo, payload_bytes, nullptr, payload_bytes,
                                       out.data() + lo * frame, frame, chunk_frames);
        }, n_frames, "ofdm_tx_encode_host");
        return out;
    }

  private:
    template <class F> void run(F &&shard, int64_t n_frames, const char *what) {
        const size_t R = ctx_.size();
        std::vector<int> rc(R, OFDM_OK);
        std::vector<std::thread> th;
        th.reserve(R); // no reallocation while threads run
        struct Joiner { // whatever happens below (std::thread's constructor can throw), started shards are joined before the stack unwinds:
            std::vector<std::thread> &t; // a joinable std::thread destroyed means std::terminate with GPU work in flight
            ~Joiner() { for (auto &x : t) if (x.joinable()) x.join(); }
        } joiner{th};
        for (size_t i = 0; i < R; ++i) {
            const auto [lo, hi] = shard_range(n_frames, (int64_t)i, (int64_t)R);
            if (hi > lo) th.emplace_back([&, i, lo = lo, hi = hi] { rc[i] = shard(i, lo, hi); }); // every entry point selects its context's device itself
        }
        for (auto &t : th) t.join();
        for (int v : rc) check(v, what);
    }
    std::vector<std::unique_ptr<Context>> ctx_;
};

// outer Reed-Solomon(255,223) framing of the demos (src/utils.rs:97-180), host side
// EXT-9: sc16 <-> fc32 on the host (the definition in C: include/ofdm_hip.h).  narrow: *clipped (optional) = clipped components.
inline std::vector<ofdm_fc32> sc16_widen(const std::vector<ofdm_sc16> &in, float scale = OFDM_SC16_DEFAULT_SCALE) {
    std::vector<ofdm_fc32> out(in.size());
    check(ofdm_sc16_widen(in.data(), (int64_t)in.size(), scale, out.data()), "ofdm_sc16_widen");
    return out;
}
inline std::vector<ofdm_sc16> sc16_narrow(const std::vector<ofdm_fc32> &in, float scale = 1.0f / OFDM_SC16_DEFAULT_SCALE, int64_t *clipped = nullptr) {
    std::vector<ofdm_sc16> out(in.size());
    check(ofdm_sc16_narrow(in.data(), (int64_t)in.size(), scale, out.data(), clipped), "ofdm_sc16_narrow");
    return out;
}

inline std::vector<uint8_t> create_transmission_bytes(const std::vector<uint8_t> &data) { // utils.rs:97-136
    std::vector<uint8_t> out((size_t)ofdm_rs255_encoded_len((int64_t)data.size()));
    check(ofdm_rs255_encode(data.data(), (int64_t)data.size(), out.data()), "ofdm_rs255_encode");
    return out;
}
inline std::optional<std::vector<uint8_t>> decipher_transmission_bytes(const std::vector<uint8_t> &code) { // utils.rs:150-180
    std::vector<uint8_t> out((size_t)ofdm_rs255_decoded_len((int64_t)code.size()));
    const int rc = ofdm_rs255_decode(code.data(), (int64_t)code.size(), out.data(), nullptr);
    if (rc == OFDM_ERR_UNCORRECTABLE) return std::nullopt; // the reference returns None
    check(rc, "ofdm_rs255_decode");
    return out;
}

// CRC-32 of IEEE 802.3 / zlib, host side (the check word of the OFDM_ECC_FCS envelope)
inline uint32_t crc32(const std::vector<uint8_t> &data) { return ofdm_crc32(data.data(), (int64_t)data.size()); }

// LDPC(648,324) on the host (the code of OFDM_ECC_LDPC648; include/ofdm_hip.h): bytes a frame of p payload bytes carries, whole
// 40-byte blocks -> 80 code bytes each, whole code words of 640 LLRs (positive = bit 1) -> 40 bytes each
inline int64_t ldpc648_coded_len(int64_t payload_bytes) { return ofdm_ldpc648_coded_len(payload_bytes); }
inline std::vector<uint8_t> ldpc648_encode(const std::vector<uint8_t> &info) {
    if (info.size() % 40) throw Error("ldpc648_encode: whole 40-byte blocks expected");
    std::vector<uint8_t> out(2 * info.size());
    check(ofdm_ldpc648_encode(info.data(), (int64_t)(info.size() / 40), out.data()), "ofdm_ldpc648_encode");
    return out;
}
inline std::vector<uint8_t> ldpc648_decode(const std::vector<int8_t> &llr, int32_t max_iter = OFDM_LDPC_MAX_ITER, std::vector<int32_t> *iters = nullptr) {
    if (llr.size() % 640) throw Error("ldpc648_decode: whole code words of 640 LLRs expected");
    std::vector<uint8_t> out(llr.size() / 16);
    if (iters) iters->resize(llr.size() / 640);
    check(ofdm_ldpc648_decode(llr.data(), (int64_t)(llr.size() / 640), max_iter, out.data(), iters ? iters->data() : nullptr), "ofdm_ldpc648_decode");
    return out;
}

// ... and over the family (rate 0 = 1/2, 1 = 2/3, 2 = 3/4, 3 = 5/6: the codes of OFDM_ECC_LDPC648 / _R23 / _R34 / _R56), K = ldpc648_info_bytes(rate)
inline int32_t ldpc648_info_bytes(int32_t rate) {
    const int32_t k = ofdm_ldpc648_info_bytes(rate);
    if (k <= 0) throw Error("ldpc648_info_bytes: rate must be 0 .. 3");
    return k;
}
inline int64_t ldpc648_coded_len(int64_t payload_bytes, int32_t rate) { return ofdm_ldpc648_coded_len_rate(payload_bytes, rate); }
inline std::vector<uint8_t> ldpc648_encode(const std::vector<uint8_t> &info, int32_t rate) {
    const size_t k = (size_t)ldpc648_info_bytes(rate);
    if (info.size() % k) throw Error("ldpc648_encode: whole blocks of K info bytes expected");
    std::vector<uint8_t> out(80 * (info.size() / k));
    check(ofdm_ldpc648_encode_rate(info.data(), (int64_t)(info.size() / k), rate, out.data()), "ofdm_ldpc648_encode_rate");
    return out;
}
inline std::vector<uint8_t> ldpc648_decode(const std::vector<int8_t> &llr, int32_t max_iter, int32_t rate, std::vector<int32_t> *iters = nullptr) {
    const size_t k = (size_t)ldpc648_info_bytes(rate);
    if (llr.size() % 640) throw Error("ldpc648_decode: whole code words of 640 LLRs expected");
    std::vector<uint8_t> out(k * (llr.size() / 640));
    if (iters) iters->resize(llr.size() / 640);
    check(ofdm_ldpc648_decode_rate(llr.data(), (int64_t)(llr.size() / 640), max_iter, rate, out.data(), iters ? iters->data() : nullptr),
          "ofdm_ldpc648_decode_rate");
    return out;
}

// utils::Analysis (src/utils.rs:38-69)
struct Analysis {
    uint32_t num_errs = 0, num_block_errs = 0;
    double err_rate = 0.0;
    Analysis(const std::vector<uint8_t> &l, const std::vector<uint8_t> &r) {
        if (l.size() != r.size()) throw Error("Analysis: length mismatch");
        for (size_t i = 0; i < l.size(); ++i)
            if (l[i] != r[i]) { num_errs += (uint32_t)__builtin_popcount((unsigned)(l[i] ^ r[i])); num_block_errs++; }
        err_rate = l.empty() ? 0.0 : (double)num_errs / ((double)l.size() * 8.0);
    }
};

} // namespace ofdm
