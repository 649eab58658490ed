// ofdm_host_path.hip -- the host-buffer side of the C ABI (include/ofdm_hip.h, "host buffers" and "one long capture").
//
// The reference's encode / decode own HOST vectors (encode returns a Vec<Complex64>, src/transmitter.rs:11-15; decode consumes one,
// src/receiver.rs:9-13) and its receiver example hands ONE 2 M-sample buffer to each decode! (examples/jetson_rx.rs:15-17,48-49,
// 84-86).  The device-buffer entry points of ofdm_abi.hip leave staging to the caller; these do it inside the library:
//   * ofdm_rx_decode_host / ofdm_rx_demod_host / ofdm_tx_encode_host: the batch is cut into chunks that travel through three slots --
//     H2D(k+1) on a copy stream, the kernels of chunk k on the context's stream, D2H(k-1) on a second copy stream, ordered by events.
//     Pinned caller memory (ofdm_host_alloc / ofdm_host_register) is DMA-ed in place; pageable memory goes through pinned bounce
//     buffers that the calling thread fills while the previous chunk's DMA runs.
//   * ofdm_sc_correlate_long / ofdm_rx_decode_long[_host]: one long capture is searched as a BATCH of overlapping slices (own lags +
//     a read-only halo of 2W + L samples, the single-GPU form of SURVEY 8(e)'s halo split), so that a 2 M-sample buffer fills the
//     chip instead of one workgroup; the lowest slice with a threshold crossing in its OWN lags is then searched again with its whole
//     peak window, which makes the answer the one a single search over the whole capture gives.
#include "ofdm_ctx.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <exception>
#include <new>

using namespace ofdm;

namespace {
struct Buf {
    void *p = nullptr;
    size_t cap = 0;
};
} // namespace

struct HostPipe {
    static constexpr int kSlots = 3;
    hipStream_t s_in = nullptr, s_out = nullptr;
    hipEvent_t in_done[kSlots] = {}, k_done[kSlots] = {}, out_done[kSlots] = {};
    Buf d_in[kSlots], d_out[kSlots]; // device slots
    Buf h_in[kSlots], h_out[kSlots]; // pinned bounce slots
    Buf d_long;                      // device copy of one long capture (ofdm_rx_decode_long_host)
    Buf d_long16;                    // device copy of one long sc16 capture (ofdm_rx_decode_long_sc16_host)
    Buf d_scal, h_scal;              // per-slice detector outputs / per-frame scalars (device, pinned)
};

namespace {

int sync_all(ofdm_ctx *c, HostPipe *hp) {
    HIP_TRY(c, hipStreamSynchronize(hp->s_in));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipStreamSynchronize(hp->s_out));
    return OFDM_OK;
}

int dev_grow(ofdm_ctx *c, HostPipe *hp, Buf &b, size_t bytes) {
    if (bytes <= b.cap) return OFDM_OK;
    if (b.p) { int rc = sync_all(c, hp); if (rc) return rc; HIP_TRY(c, hipFree(b.p)); b.p = nullptr; b.cap = 0; }
    const size_t want = bytes + bytes / 8 + 256;
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) { c->last_hip = (int)e; b.p = nullptr; return OFDM_ERR_NOMEM; }
    b.cap = want;
    if (c->ws_poison) return poison_fill_dev(c, b.p, want, c->ws_poison & 0xFF);
    return OFDM_OK;
}
int pin_grow(ofdm_ctx *c, HostPipe *hp, Buf &b, size_t bytes) {
    if (bytes <= b.cap) return OFDM_OK;
    if (b.p) { int rc = sync_all(c, hp); if (rc) return rc; HIP_TRY(c, hipHostFree(b.p)); b.p = nullptr; b.cap = 0; }
    const size_t want = bytes + bytes / 8 + 256;
    hipError_t e = hipHostMalloc(&b.p, want, hipHostMallocDefault);
    if (e != hipSuccess) { c->last_hip = (int)e; b.p = nullptr; return OFDM_ERR_NOMEM; }
    b.cap = want;
    if (c->ws_poison) std::memset(b.p, c->ws_poison & 0xFF, want);
    return OFDM_OK;
}

int pipe_get(ofdm_ctx *c, HostPipe **out) {
    if (c->pipe) { *out = c->pipe; return OFDM_OK; }
    HostPipe *hp = new (std::nothrow) HostPipe();
    if (!hp) return OFDM_ERR_NOMEM;
    // the pipe is published only when every stream and event exists: a failed creation must not leave a half-built pipe that later
    // host calls would pick up with null streams; ofdm_host_pipe_destroy tolerates the partial one
    auto build = [&]() -> int {
        HIP_TRY(c, hipStreamCreateWithFlags(&hp->s_in, hipStreamNonBlocking));
        HIP_TRY(c, hipStreamCreateWithFlags(&hp->s_out, hipStreamNonBlocking));
        for (int s = 0; s < HostPipe::kSlots; s++) {
            HIP_TRY(c, hipEventCreateWithFlags(&hp->in_done[s], hipEventDisableTiming));
            HIP_TRY(c, hipEventCreateWithFlags(&hp->k_done[s], hipEventDisableTiming));
            HIP_TRY(c, hipEventCreateWithFlags(&hp->out_done[s], hipEventDisableTiming));
        }
        return OFDM_OK;
    };
    const int rc = build();
    c->pipe = hp;
    if (rc) { ofdm_host_pipe_destroy(c); return rc; } // frees what was created and clears c->pipe
    *out = hp;
    return OFDM_OK;
}

// Is [p, p + bytes) page-locked memory the DMA engines can read in place (hipHostMalloc / hipHostRegister)?
bool host_pinned(const void *p, size_t bytes) {
    if (!p || !bytes) return true;
    auto one = [](const void *q) {
        hipPointerAttribute_t a;
        std::memset(&a, 0, sizeof(a));
        if (hipPointerGetAttributes(&a, q) != hipSuccess) { (void)hipGetLastError(); return false; } // pageable: not an error of ours
        return a.type == hipMemoryTypeHost;
    };
    return one(p) && one(static_cast<const char *>(p) + bytes - 1);
}

// One pipelined pass over the chunks of a job.
struct PipeJob {
    int64_t n_chunks = 0;
    virtual ~PipeJob() {}
    virtual size_t in_bytes(int64_t k) const = 0;
    virtual size_t out_bytes(int64_t k) const = 0;
    virtual size_t dev_out_bytes(int64_t k) const { return out_bytes(k); } // the device slot may hold more than the block that travels
    virtual const void *in_direct(int64_t) const { return nullptr; } // non-null: pinned source, DMA-ed in place
    virtual void fill_in(int64_t, void *) const {}                   // else: pack the chunk's input into the pinned bounce slot
    virtual void *out_direct(int64_t) const { return nullptr; }      // non-null: pinned destination of the whole output block
    virtual void drain_out(int64_t, const void *) const {}           // else: scatter the bounce slot into the caller's arrays
    virtual int launch(int64_t k, void *d_in, void *d_out) = 0;      // enqueue chunk k's kernels on the context's stream
    virtual int extra_d2h(int64_t, const void *, hipStream_t) { return OFDM_OK; } // a second, small D2H of chunk k behind the block's (same stream)
};

int run_pipe(ofdm_ctx *c, PipeJob &job) {
    if (job.n_chunks <= 0) return OFDM_OK;
    HostPipe *hp;
    int rc = pipe_get(c, &hp);
    if (rc) return rc;
    size_t max_in = 0, max_out = 0, max_dev_out = 0;
    bool bounce_in = false, bounce_out = false;
    for (int64_t k : {(int64_t)0, job.n_chunks - 1}) { // every chunk but the last has chunk 0's shape
        max_in = std::max(max_in, job.in_bytes(k));
        max_out = std::max(max_out, job.out_bytes(k));
        max_dev_out = std::max(max_dev_out, job.dev_out_bytes(k));
        bounce_in = bounce_in || !job.in_direct(k);
        bounce_out = bounce_out || !job.out_direct(k);
    }
    const int slots = (int)std::min<int64_t>(HostPipe::kSlots, job.n_chunks);
    for (int s = 0; s < slots; s++) {
        if ((rc = dev_grow(c, hp, hp->d_in[s], max_in + 64))) return rc; // + 64: the frame kernels' branch-free prefetches may read a little past a row
        if ((rc = dev_grow(c, hp, hp->d_out[s], max_dev_out + 64))) return rc;
        if (bounce_in && (rc = pin_grow(c, hp, hp->h_in[s], max_in))) return rc;
        if (bounce_out && (rc = pin_grow(c, hp, hp->h_out[s], max_out))) return rc;
    }
    int64_t drained = 0;
    auto drain = [&](int64_t k) -> int { // chunk k's outputs are on the host: hand them to the caller (this also frees slot k % kSlots)
        const int s = (int)(k % HostPipe::kSlots);
        HIP_TRY(c, hipEventSynchronize(hp->out_done[s]));
        if (!job.out_direct(k)) job.drain_out(k, hp->h_out[s].p);
        return OFDM_OK;
    };
    auto body = [&]() -> int {
        for (int64_t k = 0; k < job.n_chunks; k++) {
            const int s = (int)(k % HostPipe::kSlots);
            if (k >= HostPipe::kSlots) { // the slot's previous chunk must be completely through (its D2H is the last user of the slot)
                int r = drain(k - HostPipe::kSlots);
                if (r) return r;
                drained = k - HostPipe::kSlots + 1;
            }
            const void *src = job.in_direct(k);
            if (!src) { job.fill_in(k, hp->h_in[s].p); src = hp->h_in[s].p; } // overlaps the DMA of chunk k - 1
            HIP_TRY(c, hipMemcpyAsync(hp->d_in[s].p, src, job.in_bytes(k), hipMemcpyHostToDevice, hp->s_in));
            HIP_TRY(c, hipEventRecord(hp->in_done[s], hp->s_in));
            HIP_TRY(c, hipStreamWaitEvent(c->stream, hp->in_done[s], 0));
            int r = job.launch(k, hp->d_in[s].p, hp->d_out[s].p);
            if (r) return r;
            HIP_TRY(c, hipEventRecord(hp->k_done[s], c->stream));
            HIP_TRY(c, hipStreamWaitEvent(hp->s_out, hp->k_done[s], 0));
            void *dst = job.out_direct(k);
            if (!dst) dst = hp->h_out[s].p;
            HIP_TRY(c, hipMemcpyAsync(dst, hp->d_out[s].p, job.out_bytes(k), hipMemcpyDeviceToHost, hp->s_out));
            if ((r = job.extra_d2h(k, hp->d_out[s].p, hp->s_out))) return r;
            HIP_TRY(c, hipEventRecord(hp->out_done[s], hp->s_out));
        }
        for (int64_t k = drained; k < job.n_chunks; k++) {
            int r = drain(k);
            if (r) return r;
        }
        return OFDM_OK;
    };
    rc = body();
    if (rc) sync_all(c, hp); // nothing may still be reading or writing the caller's memory when the error is returned
    return rc;
}

int64_t auto_chunk(int64_t n_frames, size_t bytes_per_frame, int64_t chunk_frames) {
    if (chunk_frames <= 0) { // ~48 MB of the large side per chunk: a millisecond of PCIe time against tens of microseconds of launches
        chunk_frames = (int64_t)((size_t)48 << 20) / (int64_t)std::max<size_t>(bytes_per_frame, 1);
        if (chunk_frames > 4) chunk_frames &= ~(int64_t)3;
    }
    return std::min(std::max<int64_t>(chunk_frames, 1), std::max<int64_t>(n_frames, 1));
}

size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// ---------------------------------------------------------------- decode(host) = ofdm_rx_decode_batch per chunk
struct DecodeJob : PipeJob {
    ofdm_ctx *c;
    const void *in;
    size_t ss = sizeof(ofdm_fc32); // bytes a sample
    int64_t n_frames, stride, frame_len, n_lags, chunk;
    int32_t max_symbols;
    uint8_t *out; int64_t out_stride;
    int32_t *out_len, *status, *offset; double *fd; float *metric;
    size_t ob; // device row bytes
    bool pinned_in;
    int64_t f0(int64_t k) const { return k * chunk; }
    int64_t m(int64_t k) const { return std::min(chunk, n_frames - k * chunk); }
    size_t in_bytes(int64_t k) const override {
        const int64_t last = f0(k) + m(k) == n_frames; // only the batch's last frame may end before its stride does
        return (size_t)((m(k) - (last ? 1 : 0)) * stride + (last ? frame_len : 0)) * ss;
    }
    size_t out_bytes(int64_t k) const override { return DecodeBlock(nullptr, (size_t)m(k), ob).bytes; }
    const void *row(int64_t k) const { return static_cast<const char *>(in) + (size_t)(f0(k) * stride) * ss; }
    const void *in_direct(int64_t k) const override { return pinned_in ? row(k) : nullptr; }
    void fill_in(int64_t k, void *p) const override { std::memcpy(p, row(k), in_bytes(k)); }
    // The pipe's jobs run the device ENTRY POINT per chunk (kept on purpose): a _host call's dispatch string is its last chunk's
    int launch(int64_t k, void *d_in, void *d_out) override {
        const DecodeBlock o(d_out, (size_t)m(k), ob);
        return ofdm_rx_decode_batch(c, static_cast<const ofdm_fc32 *>(d_in), m(k), stride, frame_len, n_lags, max_symbols, o.rows, (int64_t)ob, o.len,
                                    o.status, o.offset, o.f_delta, o.metric);
    }
    void drain_out(int64_t k, const void *p) const override {
        const size_t n = (size_t)m(k);
        const int64_t a = f0(k);
        const DecodeBlock o(p, n, ob);
        if (fd) std::memcpy(fd + a, o.f_delta, n * sizeof(*fd));
        std::memcpy(out_len + a, o.len, n * sizeof(*out_len));
        std::memcpy(status + a, o.status, n * sizeof(*status));
        if (offset) std::memcpy(offset + a, o.offset, n * sizeof(*offset));
        if (metric) std::memcpy(metric + a, o.metric, n * sizeof(*metric));
        if ((size_t)out_stride == ob) std::memcpy(out + a * out_stride, o.rows, n * ob);
        else
            for (size_t f = 0; f < n; f++) // a row holds out_len[f] meaningful bytes
                std::memcpy(out + (a + (int64_t)f) * out_stride, o.rows + f * ob, (size_t)std::min<int64_t>(std::max(o.len[f], 0), out_stride));
    }
};

// ... and ofdm_rx_decode_sc16_batch per chunk (EXT-9): 4 bytes a sample over the link, the same outputs
struct DecodeSc16Job : DecodeJob {
    float scale;
    int launch(int64_t k, void *d_in, void *d_out) override {
        const DecodeBlock o(d_out, (size_t)m(k), ob);
        return ofdm_rx_decode_sc16_batch(c, static_cast<const ofdm_sc16 *>(d_in), m(k), stride, frame_len, scale, n_lags, max_symbols, o.rows,
                                         (int64_t)ob, o.len, o.status, o.offset, o.f_delta, o.metric);
    }
};

// ---------------------------------------------------------------- rx_demod(host) = ofdm_rx_demod_batch per chunk (regular streams)
struct DemodJob : PipeJob {
    ofdm_ctx *c;
    const void *in;
    size_t ss = sizeof(ofdm_fc32); // bytes a sample
    int64_t n_frames, stride, frame_len, chunk;
    int32_t first_symbol, syms;
    uint8_t *out; int64_t out_stride;
    size_t nb;
    bool pinned_in, pinned_out;
    int64_t f0(int64_t k) const { return k * chunk; }
    int64_t m(int64_t k) const { return std::min(chunk, n_frames - k * chunk); }
    size_t in_bytes(int64_t k) const override {
        const int64_t last = f0(k) + m(k) == n_frames;
        return (size_t)((m(k) - (last ? 1 : 0)) * stride + (last ? frame_len : 0)) * ss;
    }
    size_t out_bytes(int64_t k) const override { return (size_t)m(k) * nb; }
    const void *row(int64_t k) const { return static_cast<const char *>(in) + (size_t)(f0(k) * stride) * ss; }
    const void *in_direct(int64_t k) const override { return pinned_in ? row(k) : nullptr; }
    void fill_in(int64_t k, void *p) const override { std::memcpy(p, row(k), in_bytes(k)); }
    void *out_direct(int64_t k) const override { return pinned_out ? out + f0(k) * out_stride : nullptr; }
    int launch(int64_t k, void *d_in, void *d_out) override {
        return ofdm_rx_demod_batch(c, static_cast<const ofdm_fc32 *>(d_in), m(k), stride, frame_len, first_symbol, syms, nullptr, nullptr,
                                   nullptr, 0, static_cast<uint8_t *>(d_out), (int64_t)nb, nullptr);
    }
    void drain_out(int64_t k, const void *p) const override {
        const uint8_t *rows = static_cast<const uint8_t *>(p);
        if ((size_t)out_stride == nb) { std::memcpy(out + f0(k) * out_stride, rows, (size_t)m(k) * nb); return; }
        for (int64_t f = 0; f < m(k); f++) std::memcpy(out + (f0(k) + f) * out_stride, rows + (size_t)f * nb, nb);
    }
};

struct DemodSc16Job : DemodJob { // EXT-9
    float scale;
    int launch(int64_t k, void *d_in, void *d_out) override {
        return ofdm_rx_demod_sc16_batch(c, static_cast<const ofdm_sc16 *>(d_in), m(k), stride, frame_len, scale, first_symbol, syms, nullptr,
                                        nullptr, nullptr, 0, static_cast<uint8_t *>(d_out), (int64_t)nb, nullptr);
    }
};

// ---------------------------------------------------------------- encode(host) = ofdm_tx_encode_batch per chunk
struct EncodeJob : PipeJob {
    ofdm_ctx *c;
    const uint8_t *payload; int64_t n_frames, payload_stride, chunk;
    const int32_t *lens; int32_t payload_bytes;
    ofdm_fc32 *out; int64_t out_stride, frame;
    bool pinned_out;
    int64_t f0(int64_t k) const { return k * chunk; }
    int64_t m(int64_t k) const { return std::min(chunk, n_frames - k * chunk); }
    size_t lens_bytes(int64_t k) const { return lens ? round_up(4 * (size_t)m(k), 16) : 0; }
    size_t in_bytes(int64_t k) const override { return lens_bytes(k) + (size_t)m(k) * (size_t)payload_bytes; }
    size_t out_bytes(int64_t k) const override { return (size_t)m(k) * (size_t)frame * sizeof(ofdm_fc32); }
    void fill_in(int64_t k, void *p) const override { // [lens | rows of payload_bytes]: a row is read for its own length only
        char *b = static_cast<char *>(p);
        if (lens) { // clamped to the row the library stages: a length beyond payload_bytes must not walk into the next row
            int32_t *dl = reinterpret_cast<int32_t *>(b);
            for (int64_t f = 0; f < m(k); f++) dl[f] = std::min<int32_t>(std::max<int32_t>(lens[f0(k) + f], 0), payload_bytes);
        }
        b += lens_bytes(k);
        for (int64_t f = 0; f < m(k); f++) {
            int64_t n = lens ? lens[f0(k) + f] : payload_bytes;
            n = std::min<int64_t>(std::max<int64_t>(n, 0), payload_bytes);
            std::memcpy(b + (size_t)f * payload_bytes, payload + (f0(k) + f) * payload_stride, (size_t)n);
        }
    }
    void *out_direct(int64_t k) const override { return pinned_out ? out + f0(k) * out_stride : nullptr; }
    int launch(int64_t k, void *d_in, void *d_out) override {
        const char *b = static_cast<const char *>(d_in);
        return ofdm_tx_encode_batch(c, reinterpret_cast<const uint8_t *>(b + lens_bytes(k)), m(k), payload_bytes,
                                    lens ? reinterpret_cast<const int32_t *>(b) : nullptr, payload_bytes, static_cast<ofdm_fc32 *>(d_out), frame);
    }
    void drain_out(int64_t k, const void *p) const override {
        const ofdm_fc32 *rows = static_cast<const ofdm_fc32 *>(p);
        if (out_stride == frame) { std::memcpy(out + f0(k) * out_stride, rows, out_bytes(k)); return; }
        for (int64_t f = 0; f < m(k); f++) std::memcpy(out + (f0(k) + f) * out_stride, rows + f * frame, (size_t)frame * sizeof(ofdm_fc32));
    }
};

// ... and ofdm_tx_encode_sc16_batch per chunk (EXT-10): 4 bytes a sample over the link.  The device slot holds [rows of `frame` sc16
// samples | pad to 16 bytes | clipped int32 per frame].  Pageable rows: the whole block comes back through the bounce slot.  Pinned rows
// are DMA-ed in place, and the counts follow on the same stream into pinned scratch (pin_clip, the whole batch) that the caller's array is
// filled from when the pipe has drained.
struct EncodeSc16Job : EncodeJob {
    float scale;
    ofdm_sc16 *out16;
    int32_t *clipped, *pin_clip;
    size_t rows_bytes(int64_t k) const { return (size_t)m(k) * (size_t)frame * sizeof(ofdm_sc16); }
    size_t clip_off(int64_t k) const { return round_up(rows_bytes(k), 16); }
    size_t dev_out_bytes(int64_t k) const override { return clip_off(k) + 4 * (size_t)m(k); }
    size_t out_bytes(int64_t k) const override { return pinned_out || !clipped ? rows_bytes(k) : dev_out_bytes(k); }
    void *out_direct(int64_t k) const override { return pinned_out ? out16 + f0(k) * out_stride : nullptr; }
    int launch(int64_t k, void *d_in, void *d_out) override {
        const char *b = static_cast<const char *>(d_in);
        char *o = static_cast<char *>(d_out);
        return ofdm_tx_encode_sc16_batch(c, reinterpret_cast<const uint8_t *>(b + lens_bytes(k)), m(k), payload_bytes,
                                         lens ? reinterpret_cast<const int32_t *>(b) : nullptr, payload_bytes, scale,
                                         reinterpret_cast<ofdm_sc16 *>(o), frame, clipped ? reinterpret_cast<int32_t *>(o + clip_off(k)) : nullptr);
    }
    int extra_d2h(int64_t k, const void *d_out, hipStream_t st) override {
        if (!pinned_out || !clipped) return OFDM_OK;
        HIP_TRY(c, hipMemcpyAsync(pin_clip + f0(k), static_cast<const char *>(d_out) + clip_off(k), 4 * (size_t)m(k), hipMemcpyDeviceToHost, st));
        return OFDM_OK;
    }
    void drain_out(int64_t k, const void *p) const override {
        const ofdm_sc16 *rows = static_cast<const ofdm_sc16 *>(p);
        if (out_stride == frame) std::memcpy(out16 + f0(k) * out_stride, rows, rows_bytes(k));
        else
            for (int64_t f = 0; f < m(k); f++) std::memcpy(out16 + (f0(k) + f) * out_stride, rows + f * frame, (size_t)frame * sizeof(ofdm_sc16));
        if (clipped) std::memcpy(clipped + f0(k), static_cast<const char *>(p) + clip_off(k), 4 * (size_t)m(k));
    }
};

// ---------------------------------------------------------------- one long capture
struct LongGeom {
    int L, W;
    int64_t valid, lo, hi, halo, own, n_full, tail_lo, tail_len;
};
// Lags [lo, hi) of a capture of n samples as n_full slices of `own` lags (frame i = samples [lo + i own, + own + halo)) and one
// tail frame [tail_lo, tail_lo + tail_len) for whatever does not make a whole slice inside the capture.
bool long_geometry(const ofdm_ctx *c, int64_t n, int64_t lag_lo, int64_t lag_hi, int64_t slice_lags, LongGeom &g) {
    g.L = c->S(); g.W = c->prm.sync_window_reps * g.L;
    g.valid = n - g.W - g.L + 1;
    g.lo = std::max<int64_t>(lag_lo, 0);
    g.hi = (lag_hi <= 0 || lag_hi > g.valid) ? g.valid : lag_hi;
    if (g.valid <= 0 || g.lo >= g.hi) return false;
    g.halo = 2LL * g.W + g.L; // W more lags (a window that opens at the last own lag) + W + L - 1 samples under the last of them, made even
    int64_t own = slice_lags;
    if (own <= 0) {
        // N = 64: the one-tile kernel's 2560-sample tile, all of it; longer periods: ~1000 slices, but never more halo than own lags
        own = g.L == 80 ? 2560 - g.halo : std::max((g.hi - g.lo) / 1024, g.halo);
    }
    own = std::max<int64_t>((own + 1) & ~(int64_t)1, 2);
    g.own = own;
    g.n_full = 0;
    const int64_t by_lags = (g.hi - g.lo) / own;
    const int64_t by_samples = (n - g.lo - g.halo) / own; // frame i ends at lo + (i + 1) own + halo <= n
    g.n_full = std::max<int64_t>(0, std::min(by_lags, by_samples));
    g.tail_lo = g.lo + g.n_full * own;
    g.tail_len = g.tail_lo < g.hi ? std::min(n - g.tail_lo, (g.hi - g.tail_lo) + g.halo) : 0;
    return true;
}

// Pass 1 of the long search: which slice holds the first threshold crossing of [lag_lo, lag_hi) among its OWN lags.  On a hit
// *hit >= 0 and *d_clip = the capture's lag of that slice's peak with the window CLIPPED to the slice's own lags, so
// d_clip - W <= first crossing <= d_clip <= true peak.  Leaves the per-slice outputs in hp->d_scal (s_fd | s_d | s_m).
struct LongHit { int64_t hit = -1, d_clip = -1, start = 0, flen = 0, own = 0, lags2 = 0, ns = 0; };
int sc_long_find(ofdm_ctx *c, HostPipe *hp, const float2 *in, int64_t n, const LongGeom &g, LongHit &h) {
    const int64_t ns = g.n_full + (g.tail_len > 0 ? 1 : 0);
    h.ns = ns;
    if (ns > 0x7fffffff) return OFDM_ERR_INVALID;
    int rc;
    if ((rc = dev_grow(c, hp, hp->d_scal, SliceRows(nullptr, (size_t)ns).bytes + 64))) return rc;
    if ((rc = pin_grow(c, hp, hp->h_scal, (size_t)ns * sizeof(int32_t) + 64))) return rc;
    const SliceRows s(hp->d_scal.p, (size_t)ns);
    // n_lags = own clips the peak window, so only "d_hat >= 0" and the bracket above are used.  One launch over every lag: a long
    // capture is mostly noise, where the two-launch search of the batch path would read everything twice.
    const int first_lags = c->tune.sc_first_lags;
    c->tune.sc_first_lags = 0;
    rc = OFDM_OK;
    if (g.n_full) rc = ofdm_abi_sc_run(c, in + g.lo, g.n_full, g.own, g.own + g.halo, g.own, s.d_hat, s.f_delta, s.metric);
    if (!rc && g.tail_len > 0)
        rc = ofdm_abi_sc_run(c, in + g.tail_lo, 1, g.tail_len, g.tail_len, g.hi - g.tail_lo, s.d_hat + g.n_full, s.f_delta + g.n_full,
                             s.metric + g.n_full);
    c->tune.sc_first_lags = first_lags;
    if (rc) return rc;
    int32_t *h_d = static_cast<int32_t *>(hp->h_scal.p);
    HIP_TRY(c, hipMemcpyAsync(h_d, s.d_hat, (size_t)ns * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int64_t i = 0; i < ns; i++)
        if (h_d[i] >= 0) { h.hit = i; break; }
    if (h.hit < 0) return OFDM_OK;
    const bool tail = h.hit == g.n_full;
    h.start = tail ? g.tail_lo : g.lo + h.hit * g.own;
    h.flen = tail ? g.tail_len : g.own + g.halo;
    h.own = tail ? g.hi - g.tail_lo : g.own;
    h.lags2 = std::min(h.own + g.W, g.valid - h.start); // the slice's lags with the whole peak window, as far as the capture has them
    h.d_clip = h.start + h_d[h.hit];
    return OFDM_OK;
}

// The detection whose first threshold crossing lies in [lag_lo, lag_hi): -1, or the capture's lag with CFO and metric.
int sc_long(ofdm_ctx *c, const float2 *in, int64_t n, int64_t lag_lo, int64_t lag_hi, int64_t slice_lags, int64_t *d_hat, double *f_delta,
            float *metric) {
    *d_hat = -1;
    if (f_delta) *f_delta = 0.0;
    if (metric) *metric = 0.f;
    LongGeom g;
    if (!long_geometry(c, n, lag_lo, lag_hi, slice_lags, g)) return OFDM_OK;
    HostPipe *hp;
    int rc = pipe_get(c, &hp);
    if (rc) return rc;
    LongHit hit;
    if ((rc = sc_long_find(c, hp, in, n, g, hit))) return rc;
    if (hit.hit < 0) return OFDM_OK;
    const SliceRows s(hp->d_scal.p, (size_t)hit.ns);
    // pass 2: that slice again with its whole peak window (a slice that ends with the capture's last lag had it in pass 1 already)
    struct { double fd; int32_t d; float m; } h;
    h.d = (int32_t)(hit.d_clip - hit.start);
    const bool again = hit.lags2 > hit.own;
    const int64_t at = again ? 0 : hit.hit;
    if (again && (rc = ofdm_abi_sc_run(c, in + hit.start, 1, hit.flen, hit.flen, hit.lags2, s.d_hat, s.f_delta, s.metric))) return rc;
    HIP_TRY(c, hipMemcpyAsync(&h.fd, s.f_delta + at, sizeof(h.fd), hipMemcpyDeviceToHost, c->stream));
    if (again) HIP_TRY(c, hipMemcpyAsync(&h.d, s.d_hat, sizeof(h.d), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&h.m, s.metric + at, sizeof(h.m), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (h.d < 0) return OFDM_OK; // cannot happen (pass 1 saw a crossing among these lags); keep "no detection" rather than a wrong lag
    *d_hat = hit.start + h.d;
    if (f_delta) *f_delta = h.fd;
    if (metric) *metric = h.m;
    return OFDM_OK;
}

// EXT-12: every detection of [lag_lo, lag_hi) under the holdoff rule (include/ofdm_hip.h): k_sc_mark + k_sc_walk + k_sc_peaks, one D2H of
// the head and the rows into pinned memory, one synchronisation.  The rows live in kWsScanRows as head {n_det, more} | d1 | d_hat |
// f_delta | metric, `cap` entries each: cap = max_det clipped to the most detections the lag range can hold.
constexpr int64_t kScanMaxSamples = (int64_t)1 << 40; // what the kernels' 64-bit sample and bit indices are held to
int sc_scan_dev(ofdm_ctx *c, const float2 *in, int64_t n, int64_t lag_lo, int64_t lag_hi, int64_t holdoff, int64_t max_det, int64_t *d1,
                int64_t *d_hat, double *f_delta, float *metric, int64_t *n_det, int32_t *more) {
    *n_det = 0;
    if (more) *more = 0;
    ScScanParams p;
    p.L = c->S(); p.W = c->prm.sync_window_reps * p.L;
    p.valid = n - p.W - p.L + 1;
    p.lag_lo = lag_lo;
    const int64_t hi = (lag_hi <= 0 || lag_hi > p.valid) ? p.valid : lag_hi;
    if (p.valid <= 0 || lag_lo >= hi) return OFDM_OK; // no valid lag: nothing can be detected
    p.n_lags = hi - lag_lo;
    p.holdoff = holdoff;
    p.det_cap = std::min<int64_t>(max_det, (p.n_lags - 1) / holdoff + 1);
    p.threshold = c->sync_threshold_f64 > 0.0 ? c->sync_threshold_f64 : (double)c->prm.sync_threshold;
    p.in = in; p.tune = &c->tune; p.trace = &c->trace;
    HostPipe *hp;
    int rc = pipe_get(c, &hp);
    if (rc) return rc;
    void *bits, *rows;
    const size_t cap = (size_t)p.det_cap, rows_bytes = ScanRows(nullptr, cap).bytes;
    if ((rc = ws_get(c, kWsScanBits, (size_t)((p.n_lags + 63) >> 6) * 8, &bits))) return rc;
    if ((rc = ws_get(c, kWsScanRows, rows_bytes, &rows))) return rc;
    if ((rc = pin_grow(c, hp, hp->h_scal, rows_bytes))) return rc;
    p.bits = static_cast<unsigned long long *>(bits);
    const ScanRows dev(rows, cap);
    p.head = dev.head; p.d1 = dev.d1; p.d_hat = dev.d_hat; p.f_delta = dev.f_delta; p.metric = dev.metric;
    if (c->tune.scan_mark_only) { // laboratory key: the kernel's time on its own, nothing is reported
        HIP_TRY(c, run_sc_mark(p, c->num_cu, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return OFDM_OK;
    }
    HIP_TRY(c, run_sc_scan(p, c->num_cu, c->stream));
    const ScanRows h(hp->h_scal.p, cap);
    HIP_TRY(c, hipMemcpyAsync(hp->h_scal.p, rows, rows_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const size_t nd = (size_t)std::min<int64_t>(std::max<int64_t>(h.head[0], 0), p.det_cap);
    *n_det = (int64_t)nd;
    if (more) *more = h.head[1] != 0;
    if (d1) std::memcpy(d1, h.d1, nd * sizeof(*d1));
    std::memcpy(d_hat, h.d_hat, nd * sizeof(*d_hat));
    if (f_delta) std::memcpy(f_delta, h.f_delta, nd * sizeof(*f_delta));
    if (metric) std::memcpy(metric, h.metric, nd * sizeof(*metric));
    return OFDM_OK;
}

int decode_long_dev(ofdm_ctx *c, const float2 *in, int64_t n, int64_t lag_lo, int64_t lag_hi, int64_t d_known, int32_t max_symbols,
                    uint8_t *out_dev, int64_t out_cap, int32_t *out_len, int32_t *status, int64_t *offset, double *f_delta,
                    float *metric) {
    *out_len = 0; *status = OFDM_FRAME_NOSYNC;
    if (offset) *offset = 0;
    if (f_delta) *f_delta = 0.0;
    if (metric) *metric = 0.f;
    HostPipe *hp;
    int rc = pipe_get(c, &hp);
    if (rc) return rc;
    int64_t start = 0, sub_lags = 0;
    LongGeom g;
    bool have_sync = false;          // lag_lo > 0: the detection comes from the slice search below, not from the chain's own search
    int64_t k_d = -1; double k_fd = 0.0; float k_m = 0.f;
    const bool whole = lag_lo == 0 && (lag_hi <= 0 || lag_hi >= n - (int64_t)(c->prm.sync_window_reps + 1) * c->S() + 1);
    const bool one_frame = whole && d_known < 0 && (!long_geometry(c, n, 0, 0, 0, g) || g.n_full == 0);
    if (c->prm.sync_mode == OFDM_SYNC_SCHMIDL_COX && !one_frame) { // (a capture no longer than one slice is one frame of the batch path)
        const Trace::Mute search(c->trace); // the dispatch string is the chain's: the slice search in front of it is left out
        // Decode from a SUB-CAPTURE that starts at or before both the first crossing d1 and the trimmed frame start
        // (peak - L - backoff): its own search finds the same crossing, window, peak and offset as the whole capture's, and every
        // length the chain derives from "samples after the trimmed start" is unchanged.  A known peak d gives d1 >= d - W; pass 1 of
        // the slice search gives a clipped peak dc with dc - W <= d1 <= dc <= peak -- enough to place the sub-capture without
        // pass 2 (the chain's own search redoes that work on a few hundred samples anyway).
        const int L = c->S(), W = c->prm.sync_window_reps * L;
        int64_t d_lo = d_known, d_hi = d_known; // bracket of the first crossing: d1 in [d_lo - W, d_hi]
        if (d_known < 0 && lag_lo > 0) {
            // A partial lag range: the frame's trimmed start (peak - L - backoff) may lie in FRONT of lag_lo, so a sub-capture that holds the
            // whole frame also holds lags the search must not see (the tail or plateau of an earlier packet would win: ADVICE r4).  The
            // slice search is exact about "first crossing in [lag_lo, lag_hi)" (both passes); the chain then runs with that timing.
            if ((rc = sc_long(c, in, n, lag_lo, lag_hi, 0, &k_d, &k_fd, &k_m))) return rc;
            if (k_d < 0) return OFDM_OK;
            have_sync = true;
            start = std::max<int64_t>(k_d - L - c->prm.sync_backoff, 0) & ~(int64_t)1;
        } else {
        if (d_known < 0) {
            if (!long_geometry(c, n, lag_lo, lag_hi, 0, g)) return OFDM_OK;
            LongHit hit;
            if ((rc = sc_long_find(c, hp, in, n, g, hit))) return rc;
            if (hit.hit < 0) return OFDM_OK;
            d_lo = d_hi = hit.d_clip;
        }
        const int64_t back = (int64_t)W + L + c->prm.sync_backoff;
        start = std::max<int64_t>(d_lo - back, 0) & ~(int64_t)1; // even: the sub-capture stays 16-byte aligned for the LDS-DMA kernels
        sub_lags = d_hi - start + W + 2;                           // covers d1 + W; the search clips it to the capture's own last lag
        }
    } else if (c->prm.sync_mode != OFDM_SYNC_SCHMIDL_COX && !whole) {
        return OFDM_ERR_UNSUPPORTED; // the reference's detector is an argmax over the whole capture (src/receiver.rs:20-25)
    }
    if ((rc = dev_grow(c, hp, hp->d_scal, 64))) return rc;
    const DecodeBlock sc(hp->d_scal.p, 1, 0); // the one frame's scalars; its row is the caller's
    const KnownSync known{(int32_t)(k_d - start), k_fd, k_m};
    const DecodeCall d{in + start, 1, n - start, n - start, have_sync ? 0 : sub_lags, max_symbols, out_dev, out_cap, sc.len, sc.status, sc.offset,
                       sc.f_delta, sc.metric, have_sync ? &known : nullptr};
    if ((rc = ofdm_abi_rx_decode(c, d))) return rc;
    alignas(8) char back[32];
    const DecodeBlock h(back, 1, 0);
    HIP_TRY(c, hipMemcpyAsync(back, hp->d_scal.p, sc.bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *out_len = *h.len; *status = *h.status;
    if (offset) *offset = (*h.status == OFDM_FRAME_BADTIMING ? 0 : start) + *h.offset;
    if (f_delta) *f_delta = *h.f_delta;
    if (metric) *metric = *h.metric;
    return OFDM_OK;
}

// One long capture, host -> dst on the device, ordered in front of the context's stream: in place from pinned memory, else in 8 MB
// pieces through two pinned bounce slots (the copy of piece k + 1 overlaps the DMA of piece k)
int long_upload(ofdm_ctx *c, HostPipe *hp, void *dst, const void *in_host, size_t bytes) {
    int rc;
    if (host_pinned(in_host, bytes)) {
        HIP_TRY(c, hipMemcpyAsync(dst, in_host, bytes, hipMemcpyHostToDevice, hp->s_in));
    } else {
        const size_t piece = (size_t)8 << 20;
        for (int s = 0; s < 2; s++)
            if ((rc = pin_grow(c, hp, hp->h_in[s], std::min(piece, bytes)))) return rc;
        int k = 0;
        for (size_t off = 0; off < bytes; off += piece, k++) {
            const int s = k & 1;
            const size_t nb = std::min(piece, bytes - off);
            if (k >= 2) HIP_TRY(c, hipEventSynchronize(hp->in_done[s]));
            std::memcpy(hp->h_in[s].p, static_cast<const char *>(in_host) + off, nb);
            HIP_TRY(c, hipMemcpyAsync(static_cast<char *>(dst) + off, hp->h_in[s].p, nb, hipMemcpyHostToDevice, hp->s_in));
            HIP_TRY(c, hipEventRecord(hp->in_done[s], hp->s_in));
        }
    }
    HIP_TRY(c, hipEventRecord(hp->in_done[2], hp->s_in));
    HIP_TRY(c, hipStreamWaitEvent(c->stream, hp->in_done[2], 0));
    return OFDM_OK;
}

// EXT-10: ofdm_rx_decode_long on an sc16 capture that is on the device: k_sc16_widen into the context's workspace kWsLongSc16 (8 bytes a
// sample beside the capture's 4; + 64: the frame kernels' branch-free prefetches may read a little past a row), then decode_long_dev
// unchanged.  The dispatch string is k_sc16_widen+ + the fc32 call's.
int decode_long_sc16_dev(ofdm_ctx *c, const ofdm_sc16 *in, int64_t n, float scale, int64_t lag_lo, int64_t lag_hi, int64_t d_known,
                         int32_t max_symbols, uint8_t *out_dev, int64_t out_cap, int32_t *out_len, int32_t *status, int64_t *offset,
                         double *f_delta, float *metric) {
    int rc;
    void *wide;
    if ((rc = ws_get(c, kWsLongSc16, (size_t)n * sizeof(ofdm_fc32) + 64, &wide))) return rc;
    Sc16Params p = sc16_params(c, 1, n, n, n, scale);
    p.sc_in = reinterpret_cast<const uint32_t *>(in); p.fc_out = static_cast<float2 *>(wide);
    HIP_TRY(c, run_sc16_widen(p, c->num_cu, c->stream));
    return decode_long_dev(c, static_cast<const float2 *>(wide), n, lag_lo, lag_hi, d_known, max_symbols, out_dev, out_cap, out_len, status, offset,
                           f_delta, metric);
}

// The long-capture _host calls: the capture into `slot` on the device (and out_bytes of d_out[0], if the call delivers a row), then
// body(hp, the device copy).  Once the upload has started, DMA reads the caller's buffer (and later writes its outputs): every failure
// waits for all of it before the error goes back, as run_pipe does
template <class Body>
int with_long_upload(ofdm_ctx *c, Buf HostPipe::*slot, const void *in_host, size_t bytes, size_t out_bytes, Body body) {
    HostPipe *hp;
    int rc = pipe_get(c, &hp);
    if (rc) return rc;
    auto work = [&]() -> int {
        if ((rc = dev_grow(c, hp, hp->*slot, bytes + 64))) return rc;
        if (out_bytes && (rc = dev_grow(c, hp, hp->d_out[0], out_bytes + 64))) return rc;
        if ((rc = long_upload(c, hp, (hp->*slot).p, in_host, bytes))) return rc;
        return body(hp, (hp->*slot).p);
    };
    rc = work();
    if (rc) sync_all(c, hp);
    return rc;
}
// ... and the one row of ofdm_rx_decode_long[_sc16]_host back from d_out[0]
int long_row_back(ofdm_ctx *c, HostPipe *hp, uint8_t *out_host, const int32_t *out_len, const int32_t *status) {
    if (*status == OFDM_FRAME_OK && *out_len > 0) {
        HIP_TRY(c, hipMemcpyAsync(out_host, hp->d_out[0].p, (size_t)*out_len, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return OFDM_OK;
}

} // namespace

extern "C" {

void ofdm_host_pipe_destroy(ofdm_ctx *c) {
    HostPipe *hp = c ? c->pipe : nullptr;
    if (!hp) return;
    if (hp->s_in) hipStreamSynchronize(hp->s_in);
    if (hp->s_out) hipStreamSynchronize(hp->s_out);
    for (int s = 0; s < HostPipe::kSlots; s++) {
        if (hp->d_in[s].p) hipFree(hp->d_in[s].p);
        if (hp->d_out[s].p) hipFree(hp->d_out[s].p);
        if (hp->h_in[s].p) hipHostFree(hp->h_in[s].p);
        if (hp->h_out[s].p) hipHostFree(hp->h_out[s].p);
        if (hp->in_done[s]) hipEventDestroy(hp->in_done[s]);
        if (hp->k_done[s]) hipEventDestroy(hp->k_done[s]);
        if (hp->out_done[s]) hipEventDestroy(hp->out_done[s]);
    }
    if (hp->d_long.p) hipFree(hp->d_long.p);
    if (hp->d_long16.p) hipFree(hp->d_long16.p);
    if (hp->d_scal.p) hipFree(hp->d_scal.p);
    if (hp->h_scal.p) hipHostFree(hp->h_scal.p);
    if (hp->s_in) hipStreamDestroy(hp->s_in);
    if (hp->s_out) hipStreamDestroy(hp->s_out);
    delete hp;
    c->pipe = nullptr;
}

// Buffer i of the pipe, in the one order everything that walks them uses: the device slots d_in[], d_out[], then d_long, d_long16, d_scal;
// the pinned slots h_in[], h_out[], then h_scal.  nullptr behind the last one
static Buf *pipe_buf(HostPipe *hp, int i, bool *pinned) {
    constexpr int S = HostPipe::kSlots;
    Buf *const single[] = {&hp->d_long, &hp->d_long16, &hp->d_scal};
    *pinned = false;
    if (i < 0) return nullptr;
    if (i < S) return &hp->d_in[i];
    if ((i -= S) < S) return &hp->d_out[i];
    if ((i -= S) < 3) return single[i];
    *pinned = true;
    if ((i -= 3) < S) return &hp->h_in[i];
    if ((i -= S) < S) return &hp->h_out[i];
    return i == S ? &hp->h_scal : nullptr;
}
int ofdm_host_pipe_buffer(const ofdm_ctx *c, int i, void **p, size_t *cap, int *pinned) {
    bool pin = false;
    HostPipe empty;
    Buf *b = pipe_buf(c->pipe ? c->pipe : &empty, i, &pin);
    if (!b) return 0;
    *p = c->pipe ? b->p : nullptr; *cap = c->pipe ? b->cap : 0; *pinned = pin;
    return 1;
}
int ofdm_host_pipe_poison(ofdm_ctx *c, int fill) {
    HostPipe *hp = c->pipe;
    if (!hp) return OFDM_OK;
    int rc = sync_all(c, hp);
    if (rc) return rc;
    bool pinned = false;
    for (int i = 0; Buf *b = pipe_buf(hp, i, &pinned); i++) {
        if (!b->p) continue;
        if (pinned) std::memset(b->p, fill, b->cap);
        else if ((rc = poison_fill_dev(c, b->p, b->cap, fill))) return rc;
    }
    return OFDM_OK;
}

int ofdm_host_alloc(size_t bytes, void **host) {
    if (!host) return OFDM_ERR_INVALID;
    *host = nullptr;
    if (hipHostMalloc(host, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); *host = nullptr; return OFDM_ERR_NOMEM; }
    return OFDM_OK;
}
int ofdm_host_free(void *host) {
    if (host && hipHostFree(host) != hipSuccess) { (void)hipGetLastError(); return OFDM_ERR_HIP; }
    return OFDM_OK;
}
int ofdm_host_register(void *host, size_t bytes) {
    if (!host || !bytes) return OFDM_ERR_INVALID;
    if (hipHostRegister(host, bytes, hipHostRegisterDefault) != hipSuccess) { (void)hipGetLastError(); return OFDM_ERR_HIP; }
    return OFDM_OK;
}
int ofdm_host_unregister(void *host) {
    if (!host) return OFDM_ERR_INVALID;
    if (hipHostUnregister(host) != hipSuccess) { (void)hipGetLastError(); return OFDM_ERR_HIP; }
    return OFDM_OK;
}
int ofdm_host_is_pinned(const void *host, size_t bytes) { return host_pinned(host, bytes) ? 1 : 0; }

// the bodies of the fc32 and sc16 (EXT-9) host calls: j carries the sample size and the launch
static int decode_host_run(ofdm_ctx *c, DecodeJob &j, const void *in_host, int64_t n_frames, int64_t frame_stride, int64_t frame_len, int64_t n_lags,
                           int32_t max_symbols, uint8_t *out_host, int64_t out_stride, int32_t *out_len_host, int32_t *status_host,
                           int32_t *offset_host, double *f_delta_host, float *metric_host, int64_t chunk_frames) {
    if (!c || n_frames < 0 || frame_len <= 0 || max_symbols <= 0 || frame_stride < 0) return OFDM_ERR_INVALID;
    if (n_frames && (!in_host || !out_host || !out_len_host || !status_host)) return OFDM_ERR_INVALID;
    if (n_frames > 1 && frame_stride < frame_len) return OFDM_ERR_INVALID; // rows of a host batch do not overlap
    const int64_t need = decode_row_bytes(c, max_symbols);
    if (out_stride < need) return OFDM_ERR_INVALID;
    if (!n_frames) return OFDM_OK;
    DeviceGuard dev_guard(c->device);
    j.c = c; j.in = in_host; j.n_frames = n_frames; j.stride = n_frames > 1 ? frame_stride : frame_len; j.frame_len = frame_len;
    j.n_lags = n_lags; j.max_symbols = max_symbols; j.out = out_host; j.out_stride = out_stride; j.out_len = out_len_host;
    j.status = status_host; j.offset = offset_host; j.fd = f_delta_host; j.metric = metric_host;
    j.ob = round_up((size_t)std::max<int64_t>(need, 4), 4);
    j.chunk = auto_chunk(n_frames, (size_t)j.stride * j.ss, chunk_frames);
    j.n_chunks = (n_frames + j.chunk - 1) / j.chunk;
    j.pinned_in = host_pinned(in_host, (size_t)((n_frames - 1) * j.stride + frame_len) * j.ss);
    return run_pipe(c, j);
}
int ofdm_rx_decode_host(ofdm_ctx *c, const ofdm_fc32 *in_host, int64_t n_frames, int64_t frame_stride, int64_t frame_len, int64_t n_lags,
                        int32_t max_symbols, uint8_t *out_host, int64_t out_stride, int32_t *out_len_host, int32_t *status_host,
                        int32_t *offset_host, double *f_delta_host, float *metric_host, int64_t chunk_frames) {
    DecodeJob j;
    return decode_host_run(c, j, in_host, n_frames, frame_stride, frame_len, n_lags, max_symbols, out_host, out_stride, out_len_host, status_host,
                           offset_host, f_delta_host, metric_host, chunk_frames);
}
int ofdm_rx_decode_sc16_host(ofdm_ctx *c, const ofdm_sc16 *in_host, int64_t n_frames, int64_t frame_stride, int64_t frame_len, float scale,
                             int64_t n_lags, int32_t max_symbols, uint8_t *out_host, int64_t out_stride, int32_t *out_len_host,
                             int32_t *status_host, int32_t *offset_host, double *f_delta_host, float *metric_host, int64_t chunk_frames) {
    if (!sc16_scale_ok(scale)) return OFDM_ERR_INVALID;
    DecodeSc16Job j;
    j.ss = sizeof(ofdm_sc16); j.scale = scale;
    return decode_host_run(c, j, in_host, n_frames, frame_stride, frame_len, n_lags, max_symbols, out_host, out_stride, out_len_host, status_host,
                           offset_host, f_delta_host, metric_host, chunk_frames);
}

static int demod_host_run(ofdm_ctx *c, DemodJob &j, const void *in_host, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                          int32_t first_symbol, int32_t syms_per_frame, uint8_t *out_host, int64_t out_stride, int64_t chunk_frames) {
    if (!c || n_frames < 0 || frame_len <= 0 || syms_per_frame < 0 || first_symbol < 0 || frame_stride < 0) return OFDM_ERR_INVALID;
    if (n_frames && syms_per_frame && (!in_host || !out_host)) return OFDM_ERR_INVALID;
    if (n_frames > 1 && frame_stride < frame_len) return OFDM_ERR_INVALID;
    const int64_t nb = (int64_t)syms_per_frame * c->bytes_per_symbol();
    if (out_stride < nb) return OFDM_ERR_INVALID;
    if (!n_frames || !syms_per_frame) return OFDM_OK;
    DeviceGuard dev_guard(c->device);
    j.c = c; j.in = in_host; j.n_frames = n_frames; j.stride = n_frames > 1 ? frame_stride : frame_len; j.frame_len = frame_len;
    j.first_symbol = first_symbol; j.syms = syms_per_frame; j.out = out_host; j.out_stride = out_stride; j.nb = (size_t)nb;
    j.chunk = auto_chunk(n_frames, (size_t)j.stride * j.ss, chunk_frames);
    j.n_chunks = (n_frames + j.chunk - 1) / j.chunk;
    j.pinned_in = host_pinned(in_host, (size_t)((n_frames - 1) * j.stride + frame_len) * j.ss);
    j.pinned_out = out_stride == nb && host_pinned(out_host, (size_t)(n_frames * nb));
    return run_pipe(c, j);
}
int ofdm_rx_demod_host(ofdm_ctx *c, const ofdm_fc32 *in_host, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                       int32_t first_symbol, int32_t syms_per_frame, uint8_t *out_host, int64_t out_stride, int64_t chunk_frames) {
    DemodJob j;
    return demod_host_run(c, j, in_host, n_frames, frame_stride, frame_len, first_symbol, syms_per_frame, out_host, out_stride, chunk_frames);
}
int ofdm_rx_demod_sc16_host(ofdm_ctx *c, const ofdm_sc16 *in_host, int64_t n_frames, int64_t frame_stride, int64_t frame_len, float scale,
                            int32_t first_symbol, int32_t syms_per_frame, uint8_t *out_host, int64_t out_stride, int64_t chunk_frames) {
    if (!sc16_scale_ok(scale)) return OFDM_ERR_INVALID;
    DemodSc16Job j;
    j.ss = sizeof(ofdm_sc16); j.scale = scale;
    return demod_host_run(c, j, in_host, n_frames, frame_stride, frame_len, first_symbol, syms_per_frame, out_host, out_stride, chunk_frames);
}

int ofdm_tx_encode_host(ofdm_ctx *c, const uint8_t *payload_host, int64_t n_frames, int64_t payload_stride, const int32_t *payload_len_host,
                        int32_t payload_bytes, ofdm_fc32 *out_host, int64_t out_stride, int64_t chunk_frames) {
    if (!c || n_frames < 0 || payload_bytes < 0 || payload_stride < 0) return OFDM_ERR_INVALID;
    if (n_frames && (!out_host || (payload_bytes && !payload_host))) return OFDM_ERR_INVALID;
    const int64_t frame = ofdm_frame_samples(c, payload_bytes);
    if (out_stride < frame) return OFDM_ERR_INVALID;
    if (!n_frames) return OFDM_OK;
    DeviceGuard dev_guard(c->device);
    EncodeJob j;
    j.c = c; j.payload = payload_host; j.n_frames = n_frames; j.payload_stride = payload_stride; j.lens = payload_len_host;
    j.payload_bytes = payload_bytes; j.out = out_host; j.out_stride = out_stride; j.frame = frame;
    j.chunk = auto_chunk(n_frames, (size_t)frame * sizeof(ofdm_fc32), chunk_frames);
    j.n_chunks = (n_frames + j.chunk - 1) / j.chunk;
    j.pinned_out = out_stride == frame && host_pinned(out_host, (size_t)(n_frames * frame) * sizeof(ofdm_fc32));
    return run_pipe(c, j);
}

int ofdm_tx_encode_sc16_host(ofdm_ctx *c, const uint8_t *payload_host, int64_t n_frames, int64_t payload_stride, const int32_t *payload_len_host,
                             int32_t payload_bytes, float scale, ofdm_sc16 *out_host, int64_t out_stride, int32_t *clipped_host,
                             int64_t chunk_frames) {
    if (!c || n_frames < 0 || payload_bytes < 0 || payload_stride < 0 || !sc16_scale_ok(scale)) return OFDM_ERR_INVALID;
    if (n_frames && (!out_host || (payload_bytes && !payload_host))) return OFDM_ERR_INVALID;
    const int64_t frame = ofdm_frame_samples(c, payload_bytes);
    if (out_stride < frame) return OFDM_ERR_INVALID;
    if (!n_frames) return OFDM_OK;
    DeviceGuard dev_guard(c->device);
    EncodeSc16Job j;
    j.c = c; j.payload = payload_host; j.n_frames = n_frames; j.payload_stride = payload_stride; j.lens = payload_len_host;
    j.payload_bytes = payload_bytes; j.out = nullptr; j.out16 = out_host; j.out_stride = out_stride; j.frame = frame;
    j.scale = scale; j.clipped = clipped_host; j.pin_clip = nullptr;
    j.chunk = auto_chunk(n_frames, (size_t)frame * sizeof(ofdm_sc16), chunk_frames);
    j.n_chunks = (n_frames + j.chunk - 1) / j.chunk;
    j.pinned_out = out_stride == frame && host_pinned(out_host, (size_t)(n_frames * frame) * sizeof(ofdm_sc16));
    if (j.pinned_out && clipped_host) {
        HostPipe *hp;
        int rc = pipe_get(c, &hp);
        if (!rc) rc = pin_grow(c, hp, hp->h_scal, 4 * (size_t)n_frames);
        if (rc) return rc;
        j.pin_clip = static_cast<int32_t *>(hp->h_scal.p);
    }
    const int rc = run_pipe(c, j);
    if (!rc && j.pin_clip) std::memcpy(clipped_host, j.pin_clip, 4 * (size_t)n_frames);
    return rc;
}

int ofdm_sc_correlate_long(ofdm_ctx *c, const ofdm_fc32 *in_dev, int64_t n_samples, int64_t lag_lo, int64_t lag_hi, int64_t slice_lags,
                           int64_t *d_hat, double *f_delta, float *metric) {
    if (!c || !d_hat || n_samples < 0 || lag_lo < 0 || slice_lags < 0 || (n_samples && !in_dev)) return OFDM_ERR_INVALID;
    EntryScope scope(c);
    return sc_long(c, reinterpret_cast<const float2 *>(in_dev), n_samples, lag_lo, lag_hi, slice_lags, d_hat, f_delta, metric);
}

// EXT-12.  What both forms check before anything touches the device
static int sc_scan_check(const ofdm_ctx *c, const void *in, int64_t n_samples, int64_t lag_lo, int64_t holdoff, int64_t max_det,
                         const int64_t *d_hat, const int64_t *n_det) {
    if (!c || !d_hat || !n_det || n_samples < 0 || lag_lo < 0 || holdoff < 1 || max_det < 0 || (n_samples && !in)) return OFDM_ERR_INVALID;
    if (c->prm.sync_mode != OFDM_SYNC_SCHMIDL_COX || n_samples > kScanMaxSamples) return OFDM_ERR_UNSUPPORTED;
    return OFDM_OK;
}
int ofdm_sc_scan_long(ofdm_ctx *c, const ofdm_fc32 *in_dev, int64_t n_samples, int64_t lag_lo, int64_t lag_hi, int64_t holdoff,
                      int64_t max_det, int64_t *d1, int64_t *d_hat, double *f_delta, float *metric, int64_t *n_det, int32_t *more) {
    const int rc = sc_scan_check(c, in_dev, n_samples, lag_lo, holdoff, max_det, d_hat, n_det);
    if (rc) return rc;
    EntryScope scope(c);
    return sc_scan_dev(c, reinterpret_cast<const float2 *>(in_dev), n_samples, lag_lo, lag_hi, holdoff, max_det, d1, d_hat, f_delta, metric,
                       n_det, more);
}
int ofdm_sc_scan_long_host(ofdm_ctx *c, const ofdm_fc32 *in_host, int64_t n_samples, int64_t lag_lo, int64_t lag_hi, int64_t holdoff,
                           int64_t max_det, int64_t *d1, int64_t *d_hat, double *f_delta, float *metric, int64_t *n_det, int32_t *more) {
    int rc = sc_scan_check(c, in_host, n_samples, lag_lo, holdoff, max_det, d_hat, n_det);
    if (rc) return rc;
    *n_det = 0;
    if (more) *more = 0;
    if (!n_samples) return OFDM_OK;
    EntryScope scope(c);
    return with_long_upload(c, &HostPipe::d_long, in_host, (size_t)n_samples * sizeof(ofdm_fc32), 0, [&](HostPipe *, const void *x) {
        return sc_scan_dev(c, static_cast<const float2 *>(x), n_samples, lag_lo, lag_hi, holdoff, max_det, d1, d_hat, f_delta, metric, n_det, more);
    });
}

// EXT-13: upload, ofdm_sc_scan_long, ofdm_rx_decode_packets with the scan's rows, one D2H of everything.  Two synchronisations whatever
// the packet count: the scan's (its rows size the decode) and the one behind the last copy.  The device results live in d_out[0] as
// offset i64 | f_delta f64 | out_len | status i32 | metric f32 (n_det each) | the output rows.
int ofdm_rx_decode_all_long_host(ofdm_ctx *c, const ofdm_fc32 *in_host, int64_t n_samples, int64_t lag_lo, int64_t lag_hi, int64_t holdoff,
                                 int64_t max_det, int32_t max_symbols, uint8_t *out_host, int64_t out_stride, int32_t *out_len, int32_t *status,
                                 int64_t *offset, double *f_delta, float *metric, int64_t *d1, int64_t *d_hat, int64_t *n_det, int32_t *more) {
    int rc = sc_scan_check(c, in_host, n_samples, lag_lo, holdoff, max_det, d_hat, n_det);
    if (rc) return rc;
    if (max_symbols <= 0 || out_stride <= 0 || (max_det && (!out_host || !out_len || !status || !f_delta || !metric))) return OFDM_ERR_INVALID;
    if (out_stride < decode_row_bytes(c, max_symbols)) return OFDM_ERR_INVALID;
    *n_det = 0;
    if (more) *more = 0;
    if (!n_samples) return OFDM_OK;
    EntryScope scope(c);
    return with_long_upload(c, &HostPipe::d_long, in_host, (size_t)n_samples * sizeof(ofdm_fc32), 0, [&](HostPipe *hp, const void *dev) -> int {
        const float2 *x = static_cast<const float2 *>(dev);
        // (f_delta and metric receive the scan's rows first: they are the decode's input, and its outputs overwrite them)
        if ((rc = sc_scan_dev(c, x, n_samples, lag_lo, lag_hi, holdoff, max_det, d1, d_hat, f_delta, metric, n_det, more))) return rc;
        const size_t nd = (size_t)*n_det, row = (size_t)out_stride;
        if (!nd) return OFDM_OK;
        if ((rc = dev_grow(c, hp, hp->d_out[0], PacketsBlock(nullptr, nd, row).bytes + 64))) return rc;
        const PacketsBlock o(hp->d_out[0].p, nd, row);
        // (the dispatch string is the scan's kernels, then the decode's)
        rc = ofdm_abi_rx_decode_packets(c, x, n_samples, (int64_t)nd, d_hat, f_delta, metric, max_symbols, o.rows, out_stride, o.len, o.status,
                                        o.offset, o.f_delta, o.metric, 0);
        if (rc) return rc;
        if (offset) HIP_TRY(c, hipMemcpyAsync(offset, o.offset, nd * sizeof(*offset), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(f_delta, o.f_delta, nd * sizeof(*f_delta), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(out_len, o.len, nd * sizeof(*out_len), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(status, o.status, nd * sizeof(*status), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(metric, o.metric, nd * sizeof(*metric), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(out_host, o.rows, nd * row, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return OFDM_OK;
    });
}

int ofdm_rx_decode_long(ofdm_ctx *c, const ofdm_fc32 *in_dev, int64_t n_samples, int64_t lag_lo, int64_t lag_hi, int64_t d_hat_known,
                        int32_t max_symbols, uint8_t *out_dev, int64_t out_cap, int32_t *out_len, int32_t *status, int64_t *offset,
                        double *f_delta, float *metric) {
    if (!c || n_samples <= 0 || lag_lo < 0 || max_symbols <= 0 || !in_dev || !out_dev || !out_len || !status) return OFDM_ERR_INVALID;
    EntryScope scope(c);
    return decode_long_dev(c, reinterpret_cast<const float2 *>(in_dev), n_samples, lag_lo, lag_hi, d_hat_known, max_symbols, out_dev, out_cap,
                           out_len, status, offset, f_delta, metric);
}

int ofdm_rx_decode_long_host(ofdm_ctx *c, const ofdm_fc32 *in_host, int64_t n_samples, int32_t max_symbols, uint8_t *out_host,
                             int64_t out_cap, int32_t *out_len, int32_t *status, int64_t *offset, double *f_delta, float *metric) {
    if (!c || n_samples <= 0 || max_symbols <= 0 || !in_host || !out_host || !out_len || !status) return OFDM_ERR_INVALID;
    EntryScope scope(c);
    return with_long_upload(c, &HostPipe::d_long, in_host, (size_t)n_samples * sizeof(ofdm_fc32), (size_t)std::max<int64_t>(out_cap, 4),
                            [&](HostPipe *hp, const void *x) {
        const int rc = decode_long_dev(c, static_cast<const float2 *>(x), n_samples, 0, 0, -1, max_symbols, static_cast<uint8_t *>(hp->d_out[0].p),
                                       out_cap, out_len, status, offset, f_delta, metric);
        return rc ? rc : long_row_back(c, hp, out_host, out_len, status);
    });
}

// EXT-10: the two long-capture calls on sc16 samples
int ofdm_rx_decode_long_sc16(ofdm_ctx *c, const ofdm_sc16 *in_dev, int64_t n_samples, float scale, int64_t lag_lo, int64_t lag_hi,
                             int64_t d_hat_known, int32_t max_symbols, uint8_t *out_dev, int64_t out_cap, int32_t *out_len, int32_t *status,
                             int64_t *offset, double *f_delta, float *metric) {
    if (!c || n_samples <= 0 || lag_lo < 0 || max_symbols <= 0 || !in_dev || !out_dev || !out_len || !status) return OFDM_ERR_INVALID;
    if (!sc16_scale_ok(scale) || (reinterpret_cast<uintptr_t>(in_dev) & 3)) return OFDM_ERR_INVALID;
    EntryScope scope(c);
    return decode_long_sc16_dev(c, in_dev, n_samples, scale, lag_lo, lag_hi, d_hat_known, max_symbols, out_dev, out_cap, out_len, status, offset,
                                f_delta, metric);
}

int ofdm_rx_decode_long_sc16_host(ofdm_ctx *c, const ofdm_sc16 *in_host, int64_t n_samples, float scale, int32_t max_symbols, uint8_t *out_host,
                                  int64_t out_cap, int32_t *out_len, int32_t *status, int64_t *offset, double *f_delta, float *metric) {
    if (!c || n_samples <= 0 || max_symbols <= 0 || !in_host || !out_host || !out_len || !status) return OFDM_ERR_INVALID;
    if (!sc16_scale_ok(scale)) return OFDM_ERR_INVALID;
    EntryScope scope(c);
    // as ofdm_rx_decode_long_host: half the bytes over the link, then the widen in front of the chain
    return with_long_upload(c, &HostPipe::d_long16, in_host, (size_t)n_samples * sizeof(ofdm_sc16), (size_t)std::max<int64_t>(out_cap, 4),
                            [&](HostPipe *hp, const void *x) {
        const int rc = decode_long_sc16_dev(c, static_cast<const ofdm_sc16 *>(x), n_samples, scale, 0, 0, -1, max_symbols,
                                            static_cast<uint8_t *>(hp->d_out[0].p), out_cap, out_len, status, offset, f_delta, metric);
        return rc ? rc : long_row_back(c, hp, out_host, out_len, status);
    });
}

} // extern "C"

// ---- EXT-15: a DC blocker in front of detection (include/ofdm_hip.h, "a DC blocker"; numpy restatement: tests/dcblock_ref.py).  The host
// functions are the definition in C++; the handle carries the state of k_dc_block (kernels_dcblock.hip) from piece to piece: the sums
// of the last M complete blocks and the raw samples of the open block, each in two copies -- a launch reads one and writes the other.
struct ofdm_dcblock {
    ofdm_ctx *c = nullptr;
    int32_t M = 0;
    int64_t max_chunk = 0;
    int64_t T = 0;              // samples pushed since create / reset
    void *state = nullptr;      // ONE allocation: ring[0] | ring[1] | open[0] | open[1]
    double2 *ring[2] = {nullptr, nullptr};
    float2 *open[2] = {nullptr, nullptr};
    int ring_cur = 0, open_cur = 0; // the copies the next launch reads
};

namespace {

int stream_dev_alloc(ofdm_ctx *c, void **p, size_t bytes) {
    const hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) { c->last_hip = (int)e; *p = nullptr; return OFDM_ERR_NOMEM; }
    return c->ws_poison ? poison_fill_dev(c, *p, bytes, c->ws_poison & 0xFF) : OFDM_OK;
}

void dcblock_free(ofdm_dcblock *f) {
    if (f->state) hipFree(f->state);
    f->state = nullptr;
}

// The definition, one whole stream: load(i) -> sample i as fc32.  Nothing is thrown across the C boundary: a stream beyond what the
// handle takes is OFDM_ERR_UNSUPPORTED, block sums that cannot be allocated are OFDM_ERR_NOMEM
template <class Load> int dc_block_host(int64_t n, int32_t M, Load load, ofdm_fc32 *out) {
    if (n > kScanMaxSamples) return OFDM_ERR_UNSUPPORTED;
    const int64_t nb = n / 64, n_blocks = (n + 63) / 64;
    std::vector<double> sum;
    try { sum.resize((size_t)nb * 2); } catch (const std::exception &) { return OFDM_ERR_NOMEM; }
    double s[2][64];
    for (int64_t j = 0; j < nb; j++) {
        for (int i = 0; i < 64; i++) { const ofdm_fc32 x = load(64 * j + i); s[0][i] = (double)x.re; s[1][i] = (double)x.im; }
        for (int w = 32; w >= 1; w >>= 1) // the balanced pairwise tree: six times s = s[0::2] + s[1::2]
            for (int i = 0; i < w; i++) { s[0][i] = s[0][2 * i] + s[0][2 * i + 1]; s[1][i] = s[1][2 * i] + s[1][2 * i + 1]; }
        sum[(size_t)j * 2] = s[0][0]; sum[(size_t)j * 2 + 1] = s[1][0];
    }
    for (int64_t j = 0; j < n_blocks; j++) {
        const int64_t lo = std::max<int64_t>(j - M, 0), end = std::min<int64_t>(64 * j + 64, n);
        if (lo == j) { for (int64_t i = 64 * j; i < end; i++) out[i] = load(i); continue; }
        double re = sum[(size_t)lo * 2], im = sum[(size_t)lo * 2 + 1];
        for (int64_t k = lo + 1; k < j; k++) { re += sum[(size_t)k * 2]; im += sum[(size_t)k * 2 + 1]; }
        const double d = 64.0 * (double)(j - lo);
        const float mre = (float)(re / d), mim = (float)(im / d);
        for (int64_t i = 64 * j; i < end; i++) { const ofdm_fc32 x = load(i); out[i].re = x.re - mre; out[i].im = x.im - mim; }
    }
    return OFDM_OK;
}

// One piece (m samples at `in`, device memory) through k_dc_block, behind the caller's entry scope
int dcblock_piece(ofdm_dcblock *f, const void *in, int64_t m, bool sc16, float scale, float2 *out) {
    if (m <= 0) return OFDM_OK; // no launch: the state and the copies the next launch reads stay what they are
    ofdm_ctx *c = f->c;
    ofdm::DcBlockParams p;
    p.tune = &c->tune; p.trace = &c->trace;
    p.in = in; p.out = out; p.n = m; p.t0 = f->T; p.scale = scale; p.blocks = f->M;
    p.ring_old = f->ring[f->ring_cur]; p.ring_new = f->ring[f->ring_cur ^ 1];
    p.open_old = f->open[f->open_cur]; p.open_new = f->open[f->open_cur ^ 1];
    HIP_TRY(c, run_dc_block(p, sc16, c->num_cu, c->stream));
    if ((f->T + m) / 64 > f->T / 64) f->ring_cur ^= 1; // the launch wrote the other ring only if it completed a block
    f->open_cur ^= 1;
    f->T += m;
    return OFDM_OK;
}

int dcblock_push(ofdm_dcblock *f, const void *in, int64_t n, size_t ss, bool sc16, float scale, ofdm_fc32 *out) {
    if (!f || !f->c || n < 0 || (n > 0 && (!in || !out)) || (sc16 && !sc16_scale_ok(scale))) return OFDM_ERR_INVALID;
    if (n == 0) return OFDM_OK;
    if (n > kScanMaxSamples || f->T > INT64_MAX / 4 - n) return OFDM_ERR_UNSUPPORTED;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(in), a1 = a0 + (size_t)n * ss, b0 = reinterpret_cast<uintptr_t>(out), b1 = b0 + (size_t)n * sizeof(ofdm_fc32);
    if (a0 < b1 && b0 < a1) return OFDM_ERR_INVALID; // a tile reads the blocks in front of it after another tile has written them
    ofdm_ctx *c = f->c;
    EntryScope scope(c);
    for (int64_t done = 0; done < n;) {
        const int64_t m = std::min(n - done, f->max_chunk);
        const Trace::Mute later(c->trace, done > 0); // the dispatch string names what a piece ran, once
        const int rc = dcblock_piece(f, static_cast<const char *>(in) + (size_t)done * ss, m, sc16, scale, reinterpret_cast<float2 *>(out) + done);
        if (rc) return rc;
        done += m;
    }
    return OFDM_OK;
}

} // namespace

extern "C" {

int ofdm_dc_block_default(int32_t n_fft, int32_t cp_len) {
    if (n_fft < 64 || n_fft > 4096 || (n_fft & (n_fft - 1)) || cp_len != n_fft / 4) return OFDM_ERR_INVALID;
    return (3 * (n_fft + cp_len) + 63) / 64;
}

int ofdm_dc_block(const ofdm_fc32 *in, int64_t n, int32_t blocks, ofdm_fc32 *out) {
    if (n < 0 || blocks < 1 || blocks > ofdm::kDcMaxBlocks || (n > 0 && (!in || !out))) return OFDM_ERR_INVALID;
    return dc_block_host(n, blocks, [&](int64_t i) { return in[i]; }, out);
}

int ofdm_dc_block_sc16(const ofdm_sc16 *in, int64_t n, float scale, int32_t blocks, ofdm_fc32 *out) {
    if (n < 0 || blocks < 1 || blocks > ofdm::kDcMaxBlocks || (n > 0 && (!in || !out)) || !sc16_scale_ok(scale)) return OFDM_ERR_INVALID;
    // widened as it is read, by EXT-9's own host rule (one rounded product, made in another translation unit: nothing contracts it)
    return dc_block_host(n, blocks, [&](int64_t i) { ofdm_fc32 x; ofdm::sc16_widen_host(&in[i].re, 1, scale, &x.re); return x; }, out);
}

int ofdm_dcblock_create(ofdm_dcblock **out, ofdm_ctx *c, int32_t blocks, int64_t max_chunk) {
    if (out) *out = nullptr;
    if (!out || !c || blocks < 1 || blocks > ofdm::kDcMaxBlocks || max_chunk <= 0) return OFDM_ERR_INVALID;
    if (max_chunk > kScanMaxSamples) return OFDM_ERR_UNSUPPORTED;
    ofdm_dcblock *f = new (std::nothrow) ofdm_dcblock();
    if (!f) return OFDM_ERR_NOMEM;
    f->c = c; f->M = blocks; f->max_chunk = max_chunk;
    DeviceGuard dev_guard(c->device);
    const size_t ring_bytes = (size_t)blocks * sizeof(double2), open_bytes = 64 * sizeof(float2);
    const int rc = stream_dev_alloc(c, &f->state, 2 * ring_bytes + 2 * open_bytes);
    if (rc) { delete f; return rc; }
    char *b = static_cast<char *>(f->state);
    f->ring[0] = reinterpret_cast<double2 *>(b); f->ring[1] = reinterpret_cast<double2 *>(b + ring_bytes);
    f->open[0] = reinterpret_cast<float2 *>(b + 2 * ring_bytes); f->open[1] = reinterpret_cast<float2 *>(b + 2 * ring_bytes + open_bytes);
    *out = f;
    return OFDM_OK;
}

int ofdm_dcblock_destroy(ofdm_dcblock *f) {
    if (!f || !f->c) return OFDM_ERR_INVALID;
    DeviceGuard dev_guard(f->c->device);
    const hipError_t e = hipStreamSynchronize(f->c->stream);
    dcblock_free(f);
    const int rc = e == hipSuccess ? OFDM_OK : OFDM_ERR_HIP;
    if (rc) f->c->last_hip = (int)e;
    delete f;
    return rc;
}

int ofdm_dcblock_reset(ofdm_dcblock *f) {
    if (!f) return OFDM_ERR_INVALID;
    f->T = 0; // nothing of the state is read before the launch that follows has written it
    return OFDM_OK;
}

int ofdm_dcblock_push(ofdm_dcblock *f, const ofdm_fc32 *in_dev, int64_t n, ofdm_fc32 *out_dev) {
    return dcblock_push(f, in_dev, n, sizeof(ofdm_fc32), false, 0.f, out_dev);
}

int ofdm_dcblock_push_sc16(ofdm_dcblock *f, const ofdm_sc16 *in_dev, int64_t n, float scale, ofdm_fc32 *out_dev) {
    return dcblock_push(f, in_dev, n, sizeof(ofdm_sc16), true, scale, out_dev);
}

int ofdm_dcblock_state(const ofdm_dcblock *f, int64_t *total, int32_t *blocks) {
    if (!f) return OFDM_ERR_INVALID;
    if (total) *total = f->T;
    if (blocks) *blocks = f->M;
    return OFDM_OK;
}

} // extern "C"

// ---- EXT-16: a digital down-converter (include/ofdm_hip.h, "a digital down-converter"; numpy restatement: tests/ddc_ref.py).  The host
// functions are the definition in C++; the handle carries the state of k_ddc (kernels_ddc.hip) from piece to piece: the raw samples
// behind the last output, in two copies -- a launch reads one and writes the other -- and the absolute sample index.
struct ofdm_ddc_handle {
    ofdm_ctx *c = nullptr;
    int32_t D = 0, T = 0;
    uint32_t inc = 0;           // mod 2^20
    int64_t max_chunk = 0;
    int64_t n_in = 0;           // samples pushed since create / reset
    void *state = nullptr;      // ONE allocation: taps | coarse | fine | carry[0] | carry[1]
    float *taps = nullptr;
    float2 *coarse = nullptr, *fine = nullptr;
    float2 *carry[2] = {nullptr, nullptr};
    int cur = 0;                // the copy the next launch reads
};

namespace {

// The rotor tables: formed once in f64, rounded to f32; these bytes are what the host definition uses and what a handle uploads
struct DdcRotors {
    float coarse[2048], fine[2048];
    DdcRotors() {
        const double two_pi = 6.283185307179586476925286766559;
        for (int i = 0; i < 1024; i++) {
            const double a = two_pi * (double)i / 1024.0, b = two_pi * (double)i / 1048576.0;
            coarse[2 * i] = (float)std::cos(a); coarse[2 * i + 1] = (float)std::sin(a);
            fine[2 * i] = (float)std::cos(b); fine[2 * i + 1] = (float)std::sin(b);
        }
    }
};
const DdcRotors &ddc_rotors() {
    static const DdcRotors r;
    return r;
}

bool ddc_args_ok(int32_t D, int32_t T) { return D >= 1 && D <= ofdm::kDdcMaxDecim && T >= D && T <= ofdm::kDdcMaxTaps; }

// a (x) b of the definition.  The inner product is one rounded multiply: volatile keeps it out of any contraction
inline ofdm_fc32 ddc_cmul(ofdm_fc32 a, ofdm_fc32 b) {
    volatile float m0 = a.im * b.im, m1 = a.im * b.re;
    ofdm_fc32 y;
    y.re = std::fmaf(a.re, b.re, -m0);
    y.im = std::fmaf(a.re, b.im, m1);
    return y;
}

// The definition, one whole stream: load(i) -> sample i as fc32
template <class Load> int ddc_host(int64_t n, int32_t D, uint32_t inc, const float *h, int32_t T, Load load, ofdm_fc32 *out, int64_t out_cap,
                                   int64_t *n_out) {
    if (n > kScanMaxSamples) return OFDM_ERR_UNSUPPORTED;
    const int64_t M = ofdm::ddc_out_len(n, D, T);
    if (n_out) *n_out = M;
    if (M > out_cap || (M > 0 && !out)) return OFDM_ERR_INVALID;
    if (M == 0) return OFDM_OK;
    const DdcRotors &rot = ddc_rotors();
    const ofdm_fc32 *C = reinterpret_cast<const ofdm_fc32 *>(rot.coarse), *F = reinterpret_cast<const ofdm_fc32 *>(rot.fine);
    // the mixed samples under a block of outputs at a time
    constexpr int64_t kBlock = 4096;
    std::vector<ofdm_fc32> v;
    try { v.resize((size_t)(kBlock * D + T)); } catch (const std::exception &) { return OFDM_ERR_NOMEM; }
    for (int64_t m0 = 0; m0 < M; m0 += kBlock) { // outputs m0 .. m1 - 1 from the samples m0 D .. (m1 - 1) D + T - 1
        const int64_t m1 = std::min(m0 + kBlock, M), i0 = m0 * D, span = (m1 - m0 - 1) * D + T;
        for (int64_t s = 0; s < span; s++) {
            const uint32_t p = ((uint32_t)(i0 + s) * inc) & (uint32_t)ofdm::kDdcPhaseMask; // 2^20 divides 2^32
            v[(size_t)s] = ddc_cmul(load(i0 + s), ddc_cmul(C[p >> 10], F[p & 1023]));
        }
        for (int64_t m = m0; m < m1; m++) {
            const ofdm_fc32 *w = v.data() + (m - m0) * D;
            float re = 0.f, im = 0.f;
            for (int32_t k = 0; k < T; k++) { re = std::fmaf(h[k], w[k].re, re); im = std::fmaf(h[k], w[k].im, im); }
            out[m].re = re; out[m].im = im;
        }
    }
    return OFDM_OK;
}

void ddc_free(ofdm_ddc_handle *f) {
    if (f->state) hipFree(f->state);
    f->state = nullptr;
}

// One piece (m samples at `in`, device memory) through k_ddc, behind the caller's entry scope; *n_out: what it wrote at `out`
int ddc_piece(ofdm_ddc_handle *f, const void *in, int64_t m, bool sc16, float scale, float2 *out, int64_t *n_out) {
    *n_out = 0;
    if (m <= 0) return OFDM_OK; // no launch: the carry and the copy the next launch reads stay what they are
    ofdm_ctx *c = f->c;
    ofdm::DdcParams p;
    p.tune = &c->tune; p.trace = &c->trace;
    p.in = in; p.out = out; p.n = m; p.t0 = f->n_in; p.scale = scale; p.decim = f->D; p.n_taps = f->T; p.phase_inc = f->inc;
    p.taps = f->taps; p.coarse = f->coarse; p.fine = f->fine;
    p.carry_old = f->carry[f->cur]; p.carry_new = f->carry[f->cur ^ 1];
    HIP_TRY(c, run_ddc(p, sc16, c->num_cu, c->stream));
    f->cur ^= 1;
    *n_out = ofdm::ddc_out_len(f->n_in + m, f->D, f->T) - ofdm::ddc_out_len(f->n_in, f->D, f->T);
    f->n_in += m;
    return OFDM_OK;
}

int ddc_push(ofdm_ddc_handle *f, const void *in, int64_t n, size_t ss, bool sc16, float scale, ofdm_fc32 *out, int64_t out_cap, int64_t *n_out) {
    if (n_out) *n_out = 0;
    if (!f || !f->c || n < 0 || out_cap < 0 || (n > 0 && !in) || (sc16 && !sc16_scale_ok(scale))) return OFDM_ERR_INVALID;
    if (n == 0) return OFDM_OK;
    if (n > kScanMaxSamples || f->n_in > INT64_MAX / 4 - n) return OFDM_ERR_UNSUPPORTED;
    const int64_t M = ofdm::ddc_out_len(f->n_in + n, f->D, f->T) - ofdm::ddc_out_len(f->n_in, f->D, f->T);
    if (M > out_cap || (M > 0 && !out)) return OFDM_ERR_INVALID;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(in), a1 = a0 + (size_t)n * ss, b0 = reinterpret_cast<uintptr_t>(out), b1 = b0 + (size_t)M * sizeof(ofdm_fc32);
    if ((a0 & (ss - 1)) || (b0 & 7)) return OFDM_ERR_INVALID;
    if (M > 0 && a0 < b1 && b0 < a1) return OFDM_ERR_INVALID; // a tile reads samples under its neighbour's outputs
    ofdm_ctx *c = f->c;
    EntryScope scope(c);
    int64_t given = 0;
    for (int64_t done = 0; done < n;) {
        const int64_t m = std::min(n - done, f->max_chunk);
        const Trace::Mute later(c->trace, done > 0); // the dispatch string names what a piece ran, once
        int64_t k = 0;
        const int rc = ddc_piece(f, static_cast<const char *>(in) + (size_t)done * ss, m, sc16, scale, reinterpret_cast<float2 *>(out) + given, &k);
        if (rc) return rc;
        done += m;
        given += k;
    }
    if (n_out) *n_out = given;
    return OFDM_OK;
}

} // namespace

extern "C" {

int ofdm_ddc_rotor_tables(float *coarse, float *fine) {
    if (!coarse || !fine) return OFDM_ERR_INVALID;
    const DdcRotors &r = ddc_rotors();
    std::memcpy(coarse, r.coarse, sizeof(r.coarse));
    std::memcpy(fine, r.fine, sizeof(r.fine));
    return OFDM_OK;
}

int64_t ofdm_ddc_out_len(int64_t n, int32_t decim, int32_t n_taps) {
    if (n < 0 || !ddc_args_ok(decim, n_taps)) return OFDM_ERR_INVALID;
    return ofdm::ddc_out_len(n, decim, n_taps);
}

int ofdm_ddc_inc_for(double f0, int32_t *inc) {
    if (!inc || !std::isfinite(f0) || std::fabs(f0) > 0.5) return OFDM_ERR_INVALID;
    *inc = (int32_t)((-(int64_t)std::rint(f0 * 1048576.0)) & ofdm::kDdcPhaseMask);
    return OFDM_OK;
}

int ofdm_ddc_design(int32_t decim, int32_t taps_per_phase, float *taps) {
    if (decim < 1 || decim > ofdm::kDdcMaxDecim || taps_per_phase < 1 || taps_per_phase > 64 || !taps) return OFDM_ERR_INVALID;
    const int T = decim * taps_per_phase;
    if (T == 1) { taps[0] = 1.f; return OFDM_OK; }
    const double pi = 3.14159265358979323846264338327950288;
    std::vector<double> h((size_t)T);
    double sum = 0.0;
    for (int k = 0; k < T; k++) {
        const double x = ((double)k - (double)(T - 1) / 2.0) / (double)decim;
        const double s = x == 0.0 ? 1.0 : std::sin(pi * x) / (pi * x);
        h[(size_t)k] = s * (0.54 - 0.46 * std::cos(2.0 * pi * (double)k / (double)(T - 1)));
        sum += h[(size_t)k];
    }
    for (int k = 0; k < T; k++) taps[k] = (float)(h[(size_t)k] / sum);
    return OFDM_OK;
}

int ofdm_ddc(const ofdm_fc32 *in, int64_t n, int32_t decim, int32_t phase_inc, const float *taps, int32_t n_taps, ofdm_fc32 *out, int64_t out_cap,
             int64_t *n_out) {
    if (n_out) *n_out = 0;
    if (n < 0 || out_cap < 0 || !ddc_args_ok(decim, n_taps) || !taps || (n > 0 && !in)) return OFDM_ERR_INVALID;
    return ddc_host(n, decim, (uint32_t)phase_inc & (uint32_t)ofdm::kDdcPhaseMask, taps, n_taps, [&](int64_t i) { return in[i]; }, out, out_cap, n_out);
}

int ofdm_ddc_sc16(const ofdm_sc16 *in, int64_t n, float scale, int32_t decim, int32_t phase_inc, const float *taps, int32_t n_taps, ofdm_fc32 *out,
                  int64_t out_cap, int64_t *n_out) {
    if (n_out) *n_out = 0;
    if (n < 0 || out_cap < 0 || !ddc_args_ok(decim, n_taps) || !taps || (n > 0 && !in) || !sc16_scale_ok(scale)) return OFDM_ERR_INVALID;
    // widened as it is read, by EXT-9's own host rule (one rounded product, made in another translation unit: nothing contracts it)
    return ddc_host(n, decim, (uint32_t)phase_inc & (uint32_t)ofdm::kDdcPhaseMask, taps, n_taps,
                    [&](int64_t i) { ofdm_fc32 x; ofdm::sc16_widen_host(&in[i].re, 1, scale, &x.re); return x; }, out, out_cap, n_out);
}

int ofdm_ddc_create(ofdm_ddc_handle **out, ofdm_ctx *c, int32_t decim, int32_t phase_inc, const float *taps, int32_t n_taps, int64_t max_chunk) {
    if (out) *out = nullptr;
    if (!out || !c || !ddc_args_ok(decim, n_taps) || !taps || max_chunk <= 0) return OFDM_ERR_INVALID;
    if (max_chunk > kScanMaxSamples) return OFDM_ERR_UNSUPPORTED;
    ofdm_ddc_handle *f = new (std::nothrow) ofdm_ddc_handle();
    if (!f) return OFDM_ERR_NOMEM;
    f->c = c; f->D = decim; f->T = n_taps; f->inc = (uint32_t)phase_inc & (uint32_t)ofdm::kDdcPhaseMask; f->max_chunk = max_chunk;
    DeviceGuard dev_guard(c->device);
    const size_t tap_bytes = round_up((size_t)n_taps * sizeof(float), 256), rot_bytes = 1024 * sizeof(float2);
    const size_t carry_bytes = round_up((size_t)n_taps * sizeof(float2), 256);
    int rc = stream_dev_alloc(c, &f->state, tap_bytes + 2 * rot_bytes + 2 * carry_bytes);
    if (rc) { delete f; return rc; }
    char *b = static_cast<char *>(f->state);
    f->taps = reinterpret_cast<float *>(b);
    f->coarse = reinterpret_cast<float2 *>(b + tap_bytes); f->fine = reinterpret_cast<float2 *>(b + tap_bytes + rot_bytes);
    f->carry[0] = reinterpret_cast<float2 *>(b + tap_bytes + 2 * rot_bytes); f->carry[1] = reinterpret_cast<float2 *>(b + tap_bytes + 2 * rot_bytes + carry_bytes);
    const DdcRotors &r = ddc_rotors();
    hipError_t e = hipMemcpyAsync(f->taps, taps, (size_t)n_taps * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(f->coarse, r.coarse, rot_bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(f->fine, r.fine, rot_bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream); // the caller's taps are read here and never again
    if (e != hipSuccess) { c->last_hip = (int)e; ddc_free(f); delete f; return OFDM_ERR_HIP; }
    *out = f;
    return OFDM_OK;
}

int ofdm_ddc_destroy(ofdm_ddc_handle *f) {
    if (!f || !f->c) return OFDM_ERR_INVALID;
    DeviceGuard dev_guard(f->c->device);
    const hipError_t e = hipStreamSynchronize(f->c->stream);
    ddc_free(f);
    const int rc = e == hipSuccess ? OFDM_OK : OFDM_ERR_HIP;
    if (rc) f->c->last_hip = (int)e;
    delete f;
    return rc;
}

int ofdm_ddc_reset(ofdm_ddc_handle *f) {
    if (!f) return OFDM_ERR_INVALID;
    f->n_in = 0; // nothing of the carry is read before the launch that follows has written it
    return OFDM_OK;
}

int ofdm_ddc_push(ofdm_ddc_handle *f, const ofdm_fc32 *in_dev, int64_t n, ofdm_fc32 *out_dev, int64_t out_cap, int64_t *n_out) {
    return ddc_push(f, in_dev, n, sizeof(ofdm_fc32), false, 0.f, out_dev, out_cap, n_out);
}

int ofdm_ddc_push_sc16(ofdm_ddc_handle *f, const ofdm_sc16 *in_dev, int64_t n, float scale, ofdm_fc32 *out_dev, int64_t out_cap, int64_t *n_out) {
    return ddc_push(f, in_dev, n, sizeof(ofdm_sc16), true, scale, out_dev, out_cap, n_out);
}

int ofdm_ddc_state(const ofdm_ddc_handle *f, int64_t *total_in, int64_t *total_out) {
    if (!f) return OFDM_ERR_INVALID;
    if (total_in) *total_in = f->n_in;
    if (total_out) *total_out = ofdm::ddc_out_len(f->n_in, f->D, f->T);
    return OFDM_OK;
}

} // extern "C"

// ---- EXT-14: a streaming receiver (include/ofdm_hip.h, "a streaming receiver"; numpy restatement and the proofs: tests/stream_ref.py,
// tests/test_stream_cpu.py).  The stream keeps the last samples of everything pushed in one of two device windows and, per piece of a
// push: k_stream_ingest (the carry and the new chunk into the other window, one launch), ofdm_sc_scan_long's kernels over the window
// from the lag the walk resumes at, ofdm_rx_decode_packets' chain over the detections the horizon commits.  What it allocates is its
// own (no workspace role, no slot of the host pipe); the scan and the decode use the context's workspaces as every call does.
struct ofdm_stream {
    ofdm_ctx *c = nullptr;
    int32_t max_symbols = 0;
    int64_t holdoff = 0, max_chunk = 0, first = 0;
    int64_t H = 0;              // the horizon W + (10 + max_symbols) S + 2
    int64_t win_cap = 0;        // samples a window holds: H + L + b + 2 + max_chunk
    int64_t T = 0;              // samples pushed
    int64_t B = 0;              // the stream index of win[cur][0]; even
    int64_t keep_from = 0;      // where the next ingest starts its carry (B <= keep_from <= T, even)
    int64_t lo = 0;             // the lag the walk resumes at
    int cur = 0;
    bool ended = false;
    float2 *win[2] = {nullptr, nullptr};
    void *stage = nullptr;      // one chunk as it was pushed (max_chunk fc32 samples)
    // EXT-15 (ofdm_stream_set_dc_block): the filter in front of the ingest and the fc32 chunk it writes; both made by the first setting
    // that is not 0 and kept until the stream is destroyed
    ofdm_dcblock *dc = nullptr;
    void *stage_dc = nullptr;
    int32_t dc_blocks = 0;      // the setting: 0 = off
    // EXT-16 (ofdm_stream_set_ddc): the down-converter in front of everything else and the fc32 samples it writes; made by a setting
    // that is not 0 and kept until the stream is destroyed.  With it on, a push is INPUT-rate samples; T, B, lo, H count its OUTPUT
    ofdm_ddc_handle *ddc = nullptr;
    void *stage_ddc = nullptr;
    int32_t ddc_decim = 0;      // the setting: 0 = off
    void *res_dev = nullptr, *res_pin = nullptr; // PacketsBlock of kStreamScanCap rows, device and pinned
    size_t row = 0;             // bytes of a result row there
    int64_t need = 0;           // decode_row_bytes: what a caller's row receives
    std::vector<int64_t> d1, d_hat; // one scan round, window-relative
    std::vector<double> f_delta;
    std::vector<float> metric;
    // decoded and not yet handed out
    struct Packet { int64_t offset, d1, d_hat; double f_delta; float metric; int32_t len, status; };
    std::vector<Packet> q;
    std::vector<uint8_t> q_rows; // `need` bytes a packet
    size_t q_head = 0;
};

namespace {

constexpr int64_t kStreamScanCap = 256; // detections per scan + decode round (the laboratory key stream_scan_cap lowers it)

void stream_free(ofdm_stream *s) {
    for (float2 *&w : s->win) { if (w) hipFree(w); w = nullptr; }
    if (s->stage) hipFree(s->stage);
    if (s->stage_dc) hipFree(s->stage_dc);
    if (s->dc) { dcblock_free(s->dc); delete s->dc; }
    s->dc = nullptr; s->stage_dc = nullptr;
    if (s->stage_ddc) hipFree(s->stage_ddc);
    if (s->ddc) { ddc_free(s->ddc); delete s->ddc; }
    s->ddc = nullptr; s->stage_ddc = nullptr;
    if (s->res_dev) hipFree(s->res_dev);
    if (s->res_pin) hipHostFree(s->res_pin);
    s->stage = s->res_dev = s->res_pin = nullptr;
}

void stream_rewind(ofdm_stream *s, int64_t first_sample) {
    s->first = first_sample;
    s->T = s->B = s->keep_from = s->lo = 0;
    s->ended = false;
    s->q.clear(); s->q_rows.clear(); s->q_head = 0;
    if (s->dc) s->dc->T = 0; // EXT-15: the setting stays, the history goes
    if (s->ddc) s->ddc->n_in = 0; // EXT-16: likewise
}

// Scan the window from `lo` on and decode what the horizon commits (flush: everything), round by round of at most `cap` detections;
// leaves s->lo where the next piece resumes.  *synced: the context's stream was synchronised behind the piece's last launch
int stream_scan_decode(ofdm_stream *s, bool flush, bool *synced) {
    ofdm_ctx *c = s->c;
    const float2 *win = s->win[s->cur];
    const int64_t n_w = s->T - s->B;
    const int64_t L = c->S(), W = c->prm.sync_window_reps * L, valid = s->T - W - L + 1;
    const int64_t cap = c->tune.stream_scan_cap > 0 ? std::min<int64_t>(c->tune.stream_scan_cap, kStreamScanCap) : kStreamScanCap;
    int rc;
    for (int round = 0;; round++) {
        if (valid <= 0 || s->lo >= valid) return OFDM_OK; // no lag to look at (sc_scan_dev would say the same without a launch)
        const Trace::Mute later(c->trace, round > 0); // the dispatch string names what a round ran, once
        int64_t nd = 0;
        int32_t more = 0;
        if ((rc = sc_scan_dev(c, win, n_w, s->lo - s->B, 0, s->holdoff, cap, s->d1.data(), s->d_hat.data(), s->f_delta.data(), s->metric.data(),
                              &nd, &more))) return rc;
        *synced = true;
        int64_t nc = 0; // the committed ones: a detection that is not committed defers itself and every later one
        while (nc < nd && (flush || s->B + s->d1[nc] + s->H <= s->T)) nc++;
        if (nc) {
            const PacketsBlock o(s->res_dev, (size_t)kStreamScanCap, s->row), h(s->res_pin, (size_t)kStreamScanCap, s->row);
            const size_t k = (size_t)nc;
            // (f_delta and metric hold the scan's rows: the decode's input; its outputs go to the pinned block)
            if ((rc = ofdm_abi_rx_decode_packets(c, win, n_w, nc, s->d_hat.data(), s->f_delta.data(), s->metric.data(), s->max_symbols, o.rows,
                                                 (int64_t)s->row, o.len, o.status, o.offset, o.f_delta, o.metric, s->T))) return rc;
            HIP_TRY(c, hipMemcpyAsync(h.offset, o.offset, k * sizeof(*o.offset), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipMemcpyAsync(h.f_delta, o.f_delta, k * sizeof(*o.f_delta), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipMemcpyAsync(h.len, o.len, k * sizeof(*o.len), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipMemcpyAsync(h.status, o.status, k * sizeof(*o.status), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipMemcpyAsync(h.metric, o.metric, k * sizeof(*o.metric), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipMemcpyAsync(h.rows, o.rows, k * s->row, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            const size_t at = s->q_rows.size(), need = (size_t)s->need;
            s->q_rows.resize(at + k * need);
            for (size_t i = 0; i < k; i++) {
                // window-relative -> stream-relative -> reported (a BADTIMING offset is the row's own, as in ofdm_rx_decode_long)
                const int64_t base = s->B + s->first;
                s->q.push_back({(h.status[i] == OFDM_FRAME_BADTIMING ? s->first : base) + h.offset[i], base + s->d1[i], base + s->d_hat[i],
                                h.f_delta[i], h.metric[i], h.len[i], h.status[i]});
                if (need) std::memcpy(s->q_rows.data() + at + i * need, h.rows + i * s->row, need);
            }
        }
        if (nc < nd) { s->lo = s->B + s->d1[nc]; return OFDM_OK; } // deferred: the first crossing at or after it is itself
        if (nd) s->lo = s->B + s->d1[nd - 1] + s->holdoff;
        if (!more) { s->lo = std::max(s->lo, valid); return OFDM_OK; }
    }
}

// One piece (m <= max_chunk samples at `in`, ss bytes each) through ingest, scan and decode
int stream_piece(ofdm_stream *s, const void *in, int64_t m, size_t ss, bool sc16, float scale, bool flush) {
    ofdm_ctx *c = s->c;
    bool synced = false;
    int rc;
    if (m > 0 && s->ddc_decim) { // EXT-16: m input samples become the 0 .. m / D + 1 converted ones that everything below takes in
        HIP_TRY(c, hipMemcpyAsync(s->stage, in, (size_t)m * ss, hipMemcpyHostToDevice, c->stream));
        int64_t mo = 0;
        if ((rc = ddc_piece(s->ddc, s->stage, m, sc16, scale, static_cast<float2 *>(s->stage_ddc), &mo))) return rc;
        m = mo;
        sc16 = false;
    }
    if (m > 0) {
        const int64_t drop = s->keep_from - s->B, keep = s->T - s->keep_from;
        if (drop < 0 || (drop & 1) || keep < 0 || keep + m > s->win_cap) return OFDM_ERR_INVALID; // the retention bound (tests/test_stream_cpu.py): never
        if (!s->ddc_decim) HIP_TRY(c, hipMemcpyAsync(s->stage, in, (size_t)m * ss, hipMemcpyHostToDevice, c->stream));
        const void *chunk = s->ddc_decim ? s->stage_ddc : s->stage;
        StreamIngestParams p;
        p.tune = &c->tune; p.trace = &c->trace;
        p.carry = s->win[s->cur] + drop; p.keep = keep; p.n = m; p.chunk = chunk; p.scale = scale; p.win = s->win[s->cur ^ 1];
        if (s->dc_blocks) { // EXT-15: the filtered chunk, already fc32, is what the window takes in
            if ((rc = dcblock_piece(s->dc, chunk, m, sc16, scale, static_cast<float2 *>(s->stage_dc)))) return rc;
            p.chunk = s->stage_dc;
            sc16 = false;
        }
        HIP_TRY(c, run_stream_ingest(p, sc16, c->num_cu, c->stream));
        s->cur ^= 1;
        s->B = s->keep_from;
        s->T += m;
    }
    rc = stream_scan_decode(s, flush, &synced);
    if (!rc && !synced) { // a window without a lag to scan: the upload still reads the caller's memory
        const hipError_t e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) { c->last_hip = (int)e; rc = OFDM_ERR_HIP; }
    }
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
    // retain from (lo - L - b) & ~1, clamped to what the window holds: B stays even, and every later row start lies at or behind it
    const int64_t from = std::min(std::max<int64_t>(s->lo - c->S() - c->prm.sync_backoff, s->B), s->T) & ~(int64_t)1;
    s->keep_from = std::max(from, s->B);
    return OFDM_OK;
}

int stream_push(ofdm_stream *s, const void *in, int64_t n, size_t ss, bool sc16, float scale, int32_t flush, int64_t max_pkt, uint8_t *out,
                int64_t out_stride, int32_t *out_len, int32_t *status, int64_t *offset, double *f_delta, float *metric, int64_t *d1, int64_t *d_hat,
                int64_t *n_pkt, int32_t *more) {
    if (!s || !s->c || !n_pkt || n < 0 || max_pkt < 0 || (n > 0 && !in)) return OFDM_ERR_INVALID;
    if (max_pkt && (!out || !out_len || !status || !f_delta || !metric || !d_hat)) return OFDM_ERR_INVALID;
    if (out_stride < s->need || (sc16 && !sc16_scale_ok(scale))) return OFDM_ERR_INVALID;
    *n_pkt = 0;
    if (more) *more = 0;
    const bool pending = s->q_head < s->q.size();
    if (s->ended && (n > 0 || !pending)) return OFDM_ERR_INVALID; // only the drain of a flush goes on behind it
    if (s->T + n > kScanMaxSamples) return OFDM_ERR_UNSUPPORTED;
    ofdm_ctx *c = s->c;
    if (!s->ended && (n > 0 || flush)) {
        EntryScope scope(c);
        int64_t done = 0;
        do {
            const int64_t m = std::min(n - done, s->max_chunk);
            const bool last = done + m == n;
            const Trace::Mute later(c->trace, done > 0); // the dispatch string names what a piece ran, once
            const int rc = stream_piece(s, static_cast<const char *>(in) + (size_t)done * ss, m, ss, sc16, scale, flush && last);
            if (rc) return rc;
            done += m;
        } while (done < n);
        if (flush) s->ended = true;
    }
    const int64_t k = std::min<int64_t>(max_pkt, (int64_t)(s->q.size() - s->q_head));
    for (int64_t i = 0; i < k; i++) {
        const ofdm_stream::Packet &p = s->q[s->q_head + (size_t)i];
        out_len[i] = p.len; status[i] = p.status; f_delta[i] = p.f_delta; metric[i] = p.metric; d_hat[i] = p.d_hat;
        if (offset) offset[i] = p.offset;
        if (d1) d1[i] = p.d1;
        if (s->need) std::memcpy(out + i * out_stride, s->q_rows.data() + (s->q_head + (size_t)i) * (size_t)s->need, (size_t)s->need);
    }
    s->q_head += (size_t)k;
    *n_pkt = k;
    if (s->q_head == s->q.size()) { s->q.clear(); s->q_rows.clear(); s->q_head = 0; }
    else if (more) *more = 1;
    return OFDM_OK;
}

} // namespace

extern "C" {

int ofdm_stream_create(ofdm_stream **out, ofdm_ctx *c, int32_t max_symbols, int64_t holdoff, int64_t max_chunk, int64_t first_sample) {
    if (out) *out = nullptr;
    if (!out || !c || max_symbols <= 0 || holdoff < 1 || max_chunk <= 0 || first_sample < 0) return OFDM_ERR_INVALID;
    if (c->prm.sync_mode != OFDM_SYNC_SCHMIDL_COX || max_chunk > kScanMaxSamples) return OFDM_ERR_UNSUPPORTED;
    ofdm_stream *s = new (std::nothrow) ofdm_stream();
    if (!s) return OFDM_ERR_NOMEM;
    const int64_t L = c->S(), W = c->prm.sync_window_reps * L;
    s->c = c; s->max_symbols = max_symbols; s->holdoff = holdoff; s->max_chunk = max_chunk;
    s->H = W + (10 + (int64_t)max_symbols) * L + 2;
    s->win_cap = s->H + L + c->prm.sync_backoff + 2 + max_chunk;
    s->need = decode_row_bytes(c, max_symbols);
    s->row = round_up((size_t)std::max<int64_t>(s->need, 16), 16);
    stream_rewind(s, first_sample);
    DeviceGuard dev_guard(c->device);
    auto build = [&]() -> int {
        int rc;
        HostPipe *hp;
        if ((rc = pipe_get(c, &hp))) return rc; // the scan's pinned rows live there
        const size_t win_bytes = (size_t)s->win_cap * sizeof(float2) + 256, res_bytes = PacketsBlock(nullptr, (size_t)kStreamScanCap, s->row).bytes;
        for (float2 *&w : s->win)
            if ((rc = stream_dev_alloc(c, reinterpret_cast<void **>(&w), win_bytes))) return rc;
        if ((rc = stream_dev_alloc(c, &s->stage, (size_t)max_chunk * sizeof(float2) + 256))) return rc;
        if ((rc = stream_dev_alloc(c, &s->res_dev, res_bytes))) return rc;
        const hipError_t e = hipHostMalloc(&s->res_pin, res_bytes, hipHostMallocDefault);
        if (e != hipSuccess) { c->last_hip = (int)e; s->res_pin = nullptr; return OFDM_ERR_NOMEM; }
        if (c->ws_poison) std::memset(s->res_pin, c->ws_poison & 0xFF, res_bytes);
        s->d1.resize((size_t)kStreamScanCap); s->d_hat.resize((size_t)kStreamScanCap);
        s->f_delta.resize((size_t)kStreamScanCap); s->metric.resize((size_t)kStreamScanCap);
        return OFDM_OK;
    };
    const int rc = build();
    if (rc) { stream_free(s); delete s; return rc; }
    *out = s;
    return OFDM_OK;
}

int ofdm_stream_destroy(ofdm_stream *s) {
    if (!s || !s->c) return OFDM_ERR_INVALID;
    DeviceGuard dev_guard(s->c->device);
    const hipError_t e = hipStreamSynchronize(s->c->stream);
    stream_free(s);
    const int rc = e == hipSuccess ? OFDM_OK : OFDM_ERR_HIP;
    if (rc) s->c->last_hip = (int)e;
    delete s;
    return rc;
}

int ofdm_stream_reset(ofdm_stream *s, int64_t first_sample) {
    if (!s || first_sample < 0) return OFDM_ERR_INVALID;
    stream_rewind(s, first_sample);
    return OFDM_OK;
}

int ofdm_stream_push(ofdm_stream *s, const ofdm_fc32 *in_host, int64_t n, int32_t flush, int64_t max_pkt, uint8_t *out_host, int64_t out_stride,
                     int32_t *out_len, int32_t *status, int64_t *offset, double *f_delta, float *metric, int64_t *d1, int64_t *d_hat, int64_t *n_pkt,
                     int32_t *more) {
    return stream_push(s, in_host, n, sizeof(ofdm_fc32), false, 0.f, flush, max_pkt, out_host, out_stride, out_len, status, offset, f_delta, metric,
                       d1, d_hat, n_pkt, more);
}

int ofdm_stream_push_sc16(ofdm_stream *s, const ofdm_sc16 *in_host, int64_t n, float scale, int32_t flush, int64_t max_pkt, uint8_t *out_host,
                          int64_t out_stride, int32_t *out_len, int32_t *status, int64_t *offset, double *f_delta, float *metric, int64_t *d1,
                          int64_t *d_hat, int64_t *n_pkt, int32_t *more) {
    return stream_push(s, in_host, n, sizeof(ofdm_sc16), true, scale, flush, max_pkt, out_host, out_stride, out_len, status, offset, f_delta, metric,
                       d1, d_hat, n_pkt, more);
}

int ofdm_stream_set_dc_block(ofdm_stream *s, int32_t blocks) {
    if (!s || !s->c || blocks < 0 || blocks > ofdm::kDcMaxBlocks || s->T != 0) return OFDM_ERR_INVALID;
    ofdm_ctx *c = s->c;
    if (blocks && (!s->dc || s->dc->M != blocks)) {
        DeviceGuard dev_guard(c->device);
        int rc;
        if (!s->stage_dc && (rc = stream_dev_alloc(c, &s->stage_dc, (size_t)s->max_chunk * sizeof(float2) + 256))) return rc;
        ofdm_dcblock *f = nullptr;
        if ((rc = ofdm_dcblock_create(&f, c, blocks, s->max_chunk))) return rc;
        ofdm_dcblock *old = s->dc;
        s->dc = f;
        // the old window's filter: what its destroy reports (a failed synchronise; last_hip is set) is this call's result
        if (old && (rc = ofdm_dcblock_destroy(old))) return rc;
    }
    if (s->dc) s->dc->T = 0;
    s->dc_blocks = blocks;
    return OFDM_OK;
}

int ofdm_stream_get_dc_block(const ofdm_stream *s, int32_t *blocks) {
    if (!s || !blocks) return OFDM_ERR_INVALID;
    *blocks = s->dc_blocks;
    return OFDM_OK;
}

int ofdm_stream_set_ddc(ofdm_stream *s, int32_t decim, int32_t phase_inc, const float *taps, int32_t n_taps) {
    if (!s || !s->c || s->T != 0 || (s->ddc && s->ddc->n_in != 0)) return OFDM_ERR_INVALID;
    if (decim == 0) { s->ddc_decim = 0; return OFDM_OK; }
    std::vector<float> own;
    if (!taps && n_taps == 0 && decim >= 1 && decim <= ofdm::kDdcMaxDecim) { // the default design
        try { own.resize((size_t)decim * OFDM_DDC_TAPS_PER_PHASE); } catch (const std::exception &) { return OFDM_ERR_NOMEM; }
        n_taps = decim * OFDM_DDC_TAPS_PER_PHASE;
        if (ofdm_ddc_design(decim, OFDM_DDC_TAPS_PER_PHASE, own.data())) return OFDM_ERR_INVALID;
        taps = own.data();
    }
    if (!ddc_args_ok(decim, n_taps) || !taps) return OFDM_ERR_INVALID;
    ofdm_ctx *c = s->c;
    DeviceGuard dev_guard(c->device);
    int rc;
    // a piece of max_chunk input samples gives at most max_chunk / D + 1 outputs; held for D = 1, so that a later setting fits too
    if (!s->stage_ddc && (rc = stream_dev_alloc(c, &s->stage_ddc, ((size_t)s->max_chunk + 2) * sizeof(float2) + 256))) return rc;
    ofdm_ddc_handle *f = nullptr;
    if ((rc = ofdm_ddc_create(&f, c, decim, phase_inc, taps, n_taps, s->max_chunk))) return rc;
    ofdm_ddc_handle *old = s->ddc;
    s->ddc = f;
    s->ddc_decim = decim;
    // the old setting's converter: what its destroy reports (a failed synchronise; last_hip is set) is this call's result
    if (old && (rc = ofdm_ddc_destroy(old))) return rc;
    return OFDM_OK;
}

int ofdm_stream_get_ddc(const ofdm_stream *s, int32_t *decim, int32_t *phase_inc, int32_t *n_taps) {
    if (!s) return OFDM_ERR_INVALID;
    const bool on = s->ddc_decim != 0;
    if (decim) *decim = s->ddc_decim;
    if (phase_inc) *phase_inc = on ? (int32_t)s->ddc->inc : 0;
    if (n_taps) *n_taps = on ? s->ddc->T : 0;
    return OFDM_OK;
}

int ofdm_stream_state(const ofdm_stream *s, int64_t *total, int64_t *kept_from, int64_t *next_lag, int32_t *ended) {
    if (!s) return OFDM_ERR_INVALID;
    if (total) *total = s->T;
    if (kept_from) *kept_from = s->keep_from;
    if (next_lag) *next_lag = s->lo;
    if (ended) *ended = s->ended ? 1 : 0;
    return OFDM_OK;
}

} // extern "C"
