/*
 * ofdm_hip.h -- C ABI of libofdm_hip.so: the MI355X (gfx950) OFDM modulate / demodulate hot path.
 *
 * This is the drop-in boundary for the DSP bodies of jkelleyrtp/ofdm's src/transmitter.rs and
 * src/receiver.rs.  The reference has no FFI of its own (its hot path is plain `pub fn`s re-exported
 * from src/lib.rs:8-21); each entry point below names the reference function (file:line) whose body it
 * replaces.  The Rust host keeps its signatures and calls these through `extern "C"`
 * (bindings/ofdm_hip.rs).
 *
 * Conventions
 *   - plain pointers and sizes only; no C++ or torch types; every call returns an `int` status
 *     (0 = OFDM_OK, negative = error) and never throws or aborts across the boundary.
 *   - sample buffers are interleaved IQ `fc32` = {float re, float im} (8 B), the reference's wire format
 *     (src/utils.rs:228-254).  All `dev` pointers are DEVICE pointers on the context's GPU; buffers are
 *     caller-owned.  Kernels are enqueued on the context's HIP stream and NOT synchronised: call
 *     ofdm_synchronize() (or synchronise the stream you passed in) before reading results on the host.
 *   - batch first: the reference's one-frame functions are the n_frames = 1 case.
 *   - one context per (thread, GPU); a context is not thread-safe, different contexts are independent.
 *   - CFO values are f64 rad/sample (frequency_correction returns f64, src/receiver.rs:231): an f32 CFO would
 *     cost ~1e-5 rad of phase by the end of a 2000-sample frame.
 *   - pilot tables (preamble, training) are INPUTS: the reference draws them from rand 0.8 StdRng
 *     (src/transmitter.rs:75-96), which cannot be verified offline; ofdm_default_pilots() supplies the
 *     documented SplitMix64 defaults and ofdm_stdrng_pilots() a restatement of the StdRng tables.
 *
 * Input amplitude
 *   Every receive-side definition below is homogeneous in the capture, and the library keeps it so: no threshold, trust
 *   test or slack constant in a kernel is absolute, each is relative to an energy the kernel has already summed.  Scaling
 *   a capture by a real g != 0 leaves every result what it was -- timing, status, m, CFO, the Schmidl-Cox metric, equalised
 *   points, w_k, LLRs, snr, llr_unit, evm2 and the delivered bytes -- and for g = +-2^k, where the scaling is exact in
 *   f32, bit for bit.  What scales is what is an amplitude or a power by definition: H (ofdm_estimate_channel_batch,
 *   ofdm_chest_smooth_batch) by g, the xcorr peak |out[idx_max]| (also the `metric` of a decode under OFDM_SYNC_REFERENCE)
 *   by |g|, noise_var, gain and both wide-CFO metrics by g^2.  A channel estimate passed in must belong to the capture it
 *   is passed with (hk of g x is g hk); a stage call WITHOUT one (ofdm_rx_demod_batch / ofdm_rx_llr_batch with hk = NULL,
 *   which is all the burst forms of k_demod64 serve) demaps unequalised points, which scale with g: its bytes, soft
 *   points and LLRs are not invariant.  The range the tests pin (tests/test_gpu_gain.py) is 2^-20 .. 2^20 around a
 *   frame whose peak is 1, for every kernel; beyond it f32 squares of window sums approach the subnormal / overflow ends.
 *   The `scale` of the sc16 entry points is such a gain: scale = 1.0 (raw counts, amplitudes up to 2^15) and the default
 *   2^-15 give the same results.  The transmit side normalises its own frames; ofdm_channel_batch is a test bench and
 *   is homogeneous to rounding only (the complex square root of its pseudo-variance).
 *
 * Extensions named by the north star that the reference lacks (64/256-QAM, Hamming(7,4), Schmidl-Cox,
 * N != 64) are defined in DESIGN.md section 3 and restated on the CPU in oracle/ofdm_oracle.c.
 */
#ifndef OFDM_HIP_H
#define OFDM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OFDM_HIP_ABI_VERSION 1

typedef struct ofdm_ctx ofdm_ctx;
typedef struct { float re, im; } ofdm_fc32;

/* call status */
enum {
    OFDM_OK = 0,
    OFDM_ERR_INVALID = -1,     /* bad argument / parameter combination */
    OFDM_ERR_UNSUPPORTED = -2, /* valid request this build does not implement */
    OFDM_ERR_NO_DEVICE = -3,   /* no HIP device / wrong architecture */
    OFDM_ERR_HIP = -4,         /* a HIP runtime call failed (ofdm_last_hip_error) */
    OFDM_ERR_NOMEM = -5,
    OFDM_ERR_UNCORRECTABLE = -6 /* outer RS block with more than 16 byte errors (the reference returns None) */
};

/* per-frame status written by ofdm_rx_decode_batch */
enum {
    OFDM_FRAME_OK = 0,
    OFDM_FRAME_SHORT = -1,  /* "Input not long enough, bailing early" (src/receiver.rs:27-29) */
    OFDM_FRAME_NOSYNC = -2, /* no lag reached the Schmidl-Cox threshold */
    OFDM_FRAME_BADTIMING = -3, /* OFDM_SYNC_REFERENCE: offset = lag - 1 outside the capture (the reference panics in split_off, receiver.rs:25) */
    OFDM_FRAME_HEADER = -4, /* fewer than 16 decoded bytes (reference panics in drain, receiver.rs:88) */
    OFDM_FRAME_UNCORRECTABLE = -5, /* OFDM_ECC_RS255*: an outer RS block with more than 16 byte errors (the reference returns None);
                                    * OFDM_ECC_LDPC648: a code word behind the first did not converge within OFDM_LDPC_MAX_ITER iterations */
    OFDM_FRAME_FCS = -6     /* OFDM_ECC_FCS + mode: the delivered row is not a valid envelope (length word or CRC-32 wrong); out_len 0 */
};

/* ModulationScheme (src/transmitter.rs:98-104) as bits per constellation point */
enum { OFDM_MOD_BPSK = 1, OFDM_MOD_QPSK = 2, OFDM_MOD_QAM16 = 4, OFDM_MOD_QAM64 = 6, OFDM_MOD_QAM256 = 8 };
/* ecc: OFDM_ECC_HAMMING74_SOFT transmits exactly what OFDM_ECC_HAMMING74 transmits (coded_len, data_symbols, frame_samples and the
 * samples of every encode entry point are the same); only decode differs: the 16-byte length header is still read from hard bits, the
 * coded body is decoded by maximum likelihood from int8 LLRs (see "soft decisions" below) instead of by syndrome.
 * OFDM_ECC_CONV_K7: the constraint-length-7, rate-1/2 convolutional code with generators 133 / 171 (octal) of 802.11a, DVB-T and DAB,
 * zero-terminated by one tail byte (coded_len(p) = 2 (p + 1)), decoded by the Viterbi algorithm from the same int8 LLRs (see
 * "convolutional code" below).  The values 3 and 4 are REJECTED (OFDM_ERR_INVALID), as is every value not named here.
 * OFDM_ECC_CONV_K7F_R12 / _R23 / _R34: the framed convolutional modes -- the same code over the payload at rate 1/2, 2/3 or 3/4
 * (punctured), behind a rate-1/2 coded length block that decode reads INSTEAD of the uncoded 16-byte header: coded_len(p) = 18 +
 * ceil(kept(8 (p + 1), rate) / 8) (see "punctured rates and framed modes" below).
 * OFDM_ECC_RS255 / OFDM_ECC_RS255_K7F_R12 / _R23 / _R34 = 20 + inner, inner = OFDM_ECC_NONE or OFDM_ECC_CONV_K7F_*: the reference's
 * outer Reed-Solomon(255,223) framing (create_transmission_bytes / decipher_transmission_bytes) around the inner mode's frame (see
 * "outer Reed-Solomon code on the device" below).  21 .. 29 and 33 .. 40 are rejected like every other value not named.
 * OFDM_ECC_LDPC648: the quasi-cyclic LDPC(648,324) code, rate 1/2, 40 info bytes to 80 coded bytes, behind no other header than its
 * own first code word, decoded by layered normalised min-sum from the same int8 LLRs: coded_len(p) = 80 ceil((p + 8) / 40) (see
 * "LDPC(648,324)" below).  13 .. 15 and 17 .. 19 stay rejected, as does 36 (RS outside LDPC is not a mode).
 * OFDM_ECC_LDPC648_R23 / _R34 / _R56 = 41 / 42 / 43: the same frame rule over the project's own LDPC(648) codes of rates 2/3, 3/4 and 5/6,
 * K = 53 / 60 / 67 info bytes to 80 coded bytes: coded_len(p) = 80 ceil((p + 8) / K) (see "LDPC(648), rates 2/3, 3/4 and 5/6" below).
 * 37 .. 40 and 44 .. 63 stay rejected, 61 .. 63 (RS outside them) among them.
 * OFDM_ECC_FCS + mode = 64 + mode, mode any of the fifteen values above (64, 65, 66, 69, 74, 75, 76, 80, 84, 94, 95, 96, 105, 106, 107): the
 * CRC-32 frame check around the payload of that mode (see "frame check sequence" below) -- decode delivers exactly the bytes that were
 * sent or reports the frame.  Every other value from 64 upwards is rejected. */
enum { OFDM_ECC_NONE = 0, OFDM_ECC_HAMMING74 = 1, OFDM_ECC_HAMMING74_SOFT = 2, OFDM_ECC_CONV_K7 = 5,
       OFDM_ECC_CONV_K7F_R12 = 10, OFDM_ECC_CONV_K7F_R23 = 11, OFDM_ECC_CONV_K7F_R34 = 12,
       OFDM_ECC_RS255 = 20, OFDM_ECC_RS255_K7F_R12 = 30, OFDM_ECC_RS255_K7F_R23 = 31, OFDM_ECC_RS255_K7F_R34 = 32,
       OFDM_ECC_LDPC648 = 16, OFDM_ECC_LDPC648_R23 = 41, OFDM_ECC_LDPC648_R34 = 42, OFDM_ECC_LDPC648_R56 = 43, OFDM_ECC_FCS = 64 };
/* iterations the OFDM_ECC_LDPC648* decode chains give a code word: a definition, not a tuned number */
#define OFDM_LDPC_MAX_ITER 20
/* bytes the envelope of an OFDM_ECC_FCS mode adds to a payload: the u32 length word in front, the u32 CRC-32 behind */
#define OFDM_FCS_OVERHEAD 8
/* puncturing rate of ofdm_conv_k7_*_punctured (the framed modes' body rate is OFDM_ECC_CONV_K7F_Rxx - OFDM_ECC_CONV_K7F_R12) */
enum { OFDM_CONV_RATE_1_2 = 0, OFDM_CONV_RATE_2_3 = 1, OFDM_CONV_RATE_3_4 = 2 };
/* llr_scale of the OFDM_ECC_HAMMING74_SOFT and OFDM_ECC_CONV_K7 decode chains (chosen from the measured BER curves);
 * the OFDM_ECC_CONV_K7F_* chains inherit it from OFDM_ECC_CONV_K7 */
#define OFDM_SOFT_LLR_SCALE 32.0f
/* cfo_mode.  OFF, SIGNED and ABS work with the Schmidl-Cox phase alone, which is defined modulo 2 pi / S rad/sample, S = n_fft + cp_len:
 * with cp_len = n_fft / 4 an acquisition range of +-pi / S, +-0.4 sub-carrier spacings.  WIDE resolves the whole multiples of 2 pi / S
 * from the training blocks (see "wide CFO acquisition" below): +-(OFDM_CFO_WIDE_SPAN + 0.5) 2 pi / S, +-6.8 sub-carrier spacings.
 * OFDM_SYNC_SCHMIDL_COX only; opt-in, receive side only, nothing on the wire changes.  4 and above are rejected. */
enum { OFDM_CFO_OFF = 0, OFDM_CFO_SIGNED = 1, OFDM_CFO_ABS = 2 /* ABS = reference's abs() (receiver.rs:239) */, OFDM_CFO_WIDE = 3 };
/* hypotheses m in [-SPAN, SPAN] the OFDM_CFO_WIDE decode chains test: a definition, not a tuned number */
#define OFDM_CFO_WIDE_SPAN 8
/* the largest span ofdm_cfo_wide_batch takes (m and m + S are the same hypothesis: a span near S / 2 would be meaningless) */
#define OFDM_CFO_WIDE_MAX_SPAN 32
/* timing / CFO detector of decode: the north star's Schmidl-Cox (default), or the reference's own pair -- cross-correlation
 * with the locking signal (xcorr_fft, src/signals/mod.rs:186-217; offset = idx_max - N = lag - 1, src/receiver.rs:20-25) and
 * frequency_correction on preamble repetitions 3 and 4 (src/receiver.rs:39, 231-240; always |.|) */
enum { OFDM_SYNC_SCHMIDL_COX = 0, OFDM_SYNC_REFERENCE = 1 };
/* ofdm_params.rx_path: rounds 2-4 offered a second N = 64 receive chain here (ONE_PASS = 2: timing and receive body in one kernel
 * from one LDS image).  It never beat the staged chain (7.4 against 4.5 ms per 1 M config-3 frames in round 5) and was removed;
 * the slot stays so that the struct layout does not change, and takes AUTO or STAGED (the same chain). */
enum { OFDM_RX_AUTO = 0, OFDM_RX_STAGED = 1 };
/* ofdm_params.chest_mode: the channel estimate decode works with.  LS = the reference's estimate_channel, bin by bin (default).
 * WLS = that estimate denoised by a weighted least-squares fit of cp_len taps (see "channel-estimate denoising" below): opt-in,
 * receive side only, transmit is untouched. */
enum { OFDM_CHEST_LS = 0, OFDM_CHEST_WLS = 1 };

typedef struct {
    int32_t n_fft;            /* sub-carriers: 64 (reference) .. 4096, power of two */
    int32_t cp_len;           /* cyclic prefix, must be n_fft / 4 (reference: 16) */
    int32_t modulation;       /* OFDM_MOD_* (reference default Bpsk, transmitter.rs:17) */
    int32_t guard_bands;      /* 0 / 1 (reference default false, transmitter.rs:16) */
    int32_t ecc;              /* OFDM_ECC_* applied to the payload around encode / decode */
    int32_t sync_window_reps; /* Schmidl-Cox window W = reps * (n_fft + cp_len); 1..3, default 3 */
    int32_t sync_backoff;     /* frame start = d_hat - L - backoff, default 4 */
    int32_t cfo_mode;         /* OFDM_CFO_* , default SIGNED */
    float sync_threshold;     /* packet-detect threshold on M(d), default 0.5 */
    int32_t sync_mode;        /* OFDM_SYNC_*, default SCHMIDL_COX (this slot was reserved[0] == 0: same layout, same default) */
    int32_t rx_path;          /* OFDM_RX_AUTO or OFDM_RX_STAGED: one chain exists (see above) */
    int32_t chest_mode;       /* OFDM_CHEST_*, default LS (this slot was reserved[0] == 0: same layout, same default) */
    int32_t reserved[4];      /* must be zero */
} ofdm_params;

/* ------------------------------------------------------------------ library / context */
int ofdm_abi_version(void);
const char *ofdm_strerror(int status);
int ofdm_device_count(int *count);
/* reference defaults: 64 carriers, CP 16, BPSK, no guard bands, no ECC */
int ofdm_default_params(ofdm_params *p);
/* SplitMix64 pilot tables (interleaved re,im doubles): preamble[2*(n_fft+cp)] = 0.25*U(-1,1) seed 100
 * (src/transmitter.rs:75-84), training[2*n_fft] = U(-1,1) seed 50 (src/transmitter.rs:88-96). Host call. */
int ofdm_default_pilots(int32_t n_fft, int32_t cp_len, double *preamble, double *training);
/* The reference's own tables: rand 0.8 StdRng (ChaCha12, seed_from_u64(100) / (50), gen_range(-1.0..1.0), re before im;
 * src/transmitter.rs:75-96) restated from the published algorithm.  Same layout as ofdm_default_pilots.  Needed only to
 * decode captures produced by the real Rust transmitter; UNVERIFIED against a running `rand` (none exists offline).
 * Host call. */
int ofdm_stdrng_pilots(int32_t n_fft, int32_t cp_len, double *preamble, double *training);
/* One ChaCha block (16 words out) from key[8] and state words 12..15, `rounds` = 8 / 12 / 20: exported so that the
 * published test vectors can pin the generator core. Host call. */
int ofdm_chacha_block(const uint32_t *key8, const uint32_t *words12_15, int32_t rounds, uint32_t *out16);
/* CRC-32 of IEEE 802.3 / zlib over n_bytes bytes (see "frame check sequence" below); 0 for a NULL pointer or a negative count.
 * Host call, no context: exported so that the definition can be pinned without a GPU. */
uint32_t ofdm_crc32(const uint8_t *data, int64_t n_bytes);
/* preamble / training: host pointers (interleaved doubles) or NULL for the defaults.  Every kernel and host table that reads one
 * reads the context's own (tests/pilot_cases.py, tests/test_gpu_pilots.py): the frame header and the maximum normalize starts from
 * (signed, over re and im of the ten header blocks, wherever it lies), 1 / t_k of the channel estimate, W_k = |t_k|^2 and R^-1 of the
 * denoised estimate, sum |t_k|^2 of the link quality, conj(t_k) of the wide CFO acquisition.
 * A ZERO TRAINING BIN t_k = 0 carries no information about H_k.  Under OFDM_CHEST_LS its estimate is 0 / 0: H_k is non-finite in that
 * bin and in no other, and a data carrier there demaps by the NaN rule -- a non-finite coordinate decides level 0 of its axis (BPSK
 * and QPSK: bit 0), so the carrier's bits are all 0 -- while w_k of "soft decisions" is a mean over ALL data carriers: one dead data
 * bin makes every LLR of the frame 0.  Under OFDM_CHEST_WLS the bin carries weight W_k = 0, H' is finite in every bin, and hard and
 * soft decisions are those of any other frame: the mode for tables with dead bins.  A dead PILOT bin (guard bands) makes the common
 * phase of every data symbol non-finite under OFDM_CHEST_LS.  A table that is zero on a whole band (the guard band nulled, as 802.11's
 * is) makes R of the denoised estimate singular to rounding: outside that mode's domain, and refused (ofdm_chest_matrix below).
 * device: HIP device ordinal.  stream: a hipStream_t (as void*); NULL = the device's default (null) stream,
 * which is what torch uses as its current stream unless told otherwise. */
int ofdm_create(const ofdm_params *p, const double *preamble, const double *training, int device, void *stream,
                ofdm_ctx **out);
int ofdm_destroy(ofdm_ctx *ctx);
int ofdm_set_stream(ofdm_ctx *ctx, void *stream);
/* Give the context a non-blocking stream of its own (destroyed with it): what a host that runs several contexts side by side
 * -- one thread per context, on one device or on several -- wants instead of the shared default stream ("one host
 * thread + one stream per device"; include/ofdm_host.hpp ShardedContext). */
int ofdm_use_own_stream(ofdm_ctx *ctx);
int ofdm_synchronize(ofdm_ctx *ctx);
int ofdm_last_hip_error(const ofdm_ctx *ctx); /* raw hipError_t of the last failing HIP call */
/* Which kernels served the LAST stage-level / pipeline entry point on this context: the names of the kernels its launchers
 * really enqueued, in order, joined by '+' (e.g. "k_sc_stream<regs>+k_rx_prepare+k_rxframe1024<finish>").
 * Every shape-specialised launcher has a generic fallback (k_sym<...>) for requests outside its envelope -- output rows that are not
 * 4- / 16-byte aligned, soft outputs -- with the same results; this call is how a caller (and the parity tests) tell which one ran.
 * The row contract of every batch entry point: rows are (base, stride, length); a base needs only the natural alignment of its
 * element (8 bytes for fc32 rows, 1 for byte rows), a stride is any 64-bit count of elements no smaller than the row where the entry
 * point says so, and neither changes a result: byte outputs are the same for every base and stride, float outputs the same bits
 * wherever this call names the same kernels and within the stated tolerance of the definition otherwise; nothing outside the rows is
 * written, nothing behind an input row's length is read into a result (tests/test_gpu_rows.py: padded and unaligned rows, loud
 * slack behind every input row, rows 2^31 + 8 samples and 2^32 + 48 bytes apart).
 * Returns the full length of the string (like snprintf), buf receives at most n - 1 characters. Host call. */
int ofdm_last_dispatch(const ofdm_ctx *ctx, char *buf, size_t n);
/* Per-context knobs and counters.  The library reads NO environment variable.  Keys a host legitimately needs:
 *   "grid_cap"             set/get, > 0 caps every persistent grid (0 = sized from the device); the parity tests use it to make small
 *                          batches walk many pipeline steps per workgroup
 *   "profile_build"        get: 1 in libofdm_hip_profile.so (-DOFDM_PROFILE_BUILD=1), 0 in the product build
 *   "stat_sc_slow_frames"  get: frames of the context's LAST N = 64 Schmidl-Cox search that were redone by the all-f64 kernel
 *   "stat_sc_redo_frames"  get: frames the first launch of the two-launch filter search left to the whole search
 *                          (both synchronise the stream; -1 = that search kept no such list)
 * Every other key is a laboratory switch between kernel variants (A/B measurements, profiling exits): listed and described in
 * ofdm_amd/csrc/ofdm_hip_tuning.h, NOT part of the drop-in contract, free to change between releases.  Unknown key: OFDM_ERR_INVALID;
 * a profiling key in the product build: OFDM_ERR_UNSUPPORTED.  Host calls. */
int ofdm_set_tuning(ofdm_ctx *ctx, const char *key, int64_t value);
int ofdm_get_tuning(const ofdm_ctx *ctx, const char *key, int64_t *value);

/* device-memory helpers so a host without its own HIP binding (the Rust crate) can stage buffers */
int ofdm_dev_alloc(ofdm_ctx *ctx, size_t bytes, void **dev);
int ofdm_dev_free(ofdm_ctx *ctx, void *dev);
int ofdm_memcpy_h2d(ofdm_ctx *ctx, void *dev, const void *host, size_t bytes); /* async on the ctx stream */
int ofdm_memcpy_d2h(ofdm_ctx *ctx, void *host, const void *dev, size_t bytes); /* synchronises the stream */
int ofdm_memset(ofdm_ctx *ctx, void *dev, int value, size_t bytes);

/* frame geometry for this context's parameters */
int ofdm_symbol_len(const ofdm_ctx *ctx);            /* S = n_fft + cp_len */
int ofdm_data_carriers(const ofdm_ctx *ctx);         /* 64k (no guard) or 48k */
int ofdm_bytes_per_symbol(const ofdm_ctx *ctx);      /* data_carriers * modulation / 8 */
int64_t ofdm_coded_len(const ofdm_ctx *ctx, int64_t payload_bytes);  /* after ECC (== payload when ECC off) */
int64_t ofdm_data_symbols(const ofdm_ctx *ctx, int64_t payload_bytes); /* D = ceil((16+coded)*8/bps / carriers) */
int64_t ofdm_frame_samples(const ofdm_ctx *ctx, int64_t payload_bytes); /* 10*S + D*S (transmitter.rs:22-54) */

/* ------------------------------------------------------------------ stage-level entry points
 * (mirror the reference's helper functions one to one; used by the parity tests and by hosts that
 * want to keep part of the chain on the CPU) */

/* SignalMut::fft / ifft (src/signals/mod.rs:27-58): n_vec transforms of length n_fft, unnormalised forward,
 * inverse scaled by 1/n_fft.  in == out allowed. */
int ofdm_fft_batch(ofdm_ctx *ctx, const ofdm_fc32 *in_dev, ofdm_fc32 *out_dev, int64_t n_vec, int inverse);
/* prefix_block (src/transmitter.rs:168-181): n_sym blocks of n_fft bins -> n_sym blocks of n_fft+cp samples */
int ofdm_ifft_cp_batch(ofdm_ctx *ctx, const ofdm_fc32 *freq_dev, ofdm_fc32 *out_dev, int64_t n_sym);
/* modulate + encode_block + prefix_block in one pass (src/transmitter.rs:40-53 without the frame header and without
 * normalize): a continuous byte stream -> n_sym symbols of n_fft+cp samples; n_sym * bytes_per_symbol >= n_bytes, bins
 * past the end of the stream carry 0 (transmitter.rs:158-160).  Same samples as the three staged calls. */
int ofdm_tx_symbols_batch(ofdm_ctx *ctx, const uint8_t *bytes_dev, int64_t n_bytes, ofdm_fc32 *out_dev, int64_t n_sym);
/* unprefix_block (src/receiver.rs:99-104): n_sym blocks of n_fft+cp samples -> n_sym blocks of n_fft bins */
int ofdm_unprefix_batch(ofdm_ctx *ctx, const ofdm_fc32 *in_dev, ofdm_fc32 *out_dev, int64_t n_sym);
/* modulate (src/transmitter.rs:108-140) + 16/64/256-QAM: n_bytes -> ceil(8 n_bytes / bps) points */
int ofdm_qam_map_batch(ofdm_ctx *ctx, const uint8_t *bytes_dev, int64_t n_bytes, ofdm_fc32 *out_dev);
/* demodulate (src/receiver.rs:147-190): n_sym points (multiple of 8) -> n_sym*bps/8 bytes;
 * idx_dev (optional) receives the per-point hard-decision index (bps-bit integer) */
int ofdm_qam_demap_batch(ofdm_ctx *ctx, const ofdm_fc32 *sym_dev, int64_t n_sym, uint8_t *bytes_dev,
                         uint8_t *idx_dev);
/* encode_block (src/transmitter.rs:144-165): per symbol, data_carriers points -> n_fft bins with nulls/pilots */
int ofdm_encode_block_batch(ofdm_ctx *ctx, const ofdm_fc32 *data_dev, ofdm_fc32 *bins_dev, int64_t n_sym);
/* normalize (src/transmitter.rs:183-194): per frame, divide by max(0, max re, max im) */
int ofdm_normalize_batch(ofdm_ctx *ctx, ofdm_fc32 *x_dev, int64_t n_frames, int64_t frame_stride, int64_t frame_len);
/* Hamming(7,4): 4 data bytes <-> 7 code bytes (north-star extension).
 * encode: n_bytes (zero-padded to a multiple of 4) -> ceil(n/4)*7; decode: floor(n/7)*4 bytes,
 * corrected_dev (optional uint32) accumulates the number of corrected codewords. */
int ofdm_hamming74_encode(ofdm_ctx *ctx, const uint8_t *in_dev, int64_t n_bytes, uint8_t *out_dev);
int ofdm_hamming74_decode(ofdm_ctx *ctx, const uint8_t *in_dev, int64_t n_bytes, uint8_t *out_dev,
                          uint32_t *corrected_dev);

/* Outer Reed-Solomon(255,223) framing of the demos (create_transmission_bytes / decipher_transmission_bytes,
 * src/utils.rs:97-180; reed-solomon 0.2.1: GF(2^8) 0x11d, generator 2, roots 2^0..2^31, parity after the data).
 * HOST calls on host buffers: byte-level work off the roofline, applied outside encode/decode as the reference does.
 * encode: n_bytes -> 255*(n/223 + 1) bytes (a final zero-padded block is always emitted, utils.rs:123-131);
 * decode: n_code -> 223*(n/255 + 1) bytes (the zero-padded remainder is decoded too, utils.rs:172-176), corrects up to
 * 16 bytes per block, OFDM_ERR_UNCORRECTABLE otherwise; *corrected (optional) = corrected bytes in total. */
int64_t ofdm_rs255_encoded_len(int64_t n_bytes);
int64_t ofdm_rs255_decoded_len(int64_t n_code);
int ofdm_rs255_encode(const uint8_t *data, int64_t n_bytes, uint8_t *out);
int ofdm_rs255_decode(const uint8_t *code, int64_t n_code, uint8_t *out, int32_t *corrected);

/* Schmidl-Cox sliding autocorrelation (north-star extension replacing xcorr_fft timing, receiver.rs:20-25).
 * Frame f occupies in_dev[f*frame_stride .. +frame_len).  Lags d in [0, n_lags) (n_lags <= 0: every lag with
 * d + W + L <= frame_len).  d_hat = first max of M over [d1, d1+W], d1 = first lag with M >= threshold;
 * d_hat[f] = -1 if none.  f_delta[f] = arg P(d_hat)/L (signed, rad/sample), metric[f] = M(d_hat).
 * That estimate is defined modulo 2 pi / L only: f_delta lies in [-pi / L, pi / L], +-0.4 sub-carrier spacings with cp_len = n_fft / 4,
 * and an offset beyond it comes back wrapped into that range with the same metric ("wide CFO acquisition" below resolves it).
 * n_lags bounds the peak window too: it is [d1, min(d1 + W, n_lags - 1)], so a bounded search returns an earlier lag than the
 * full one whenever the true peak lies beyond n_lags - 1 (same rule in the oracle; tests: test_bounded_search_clips_the_peak_window).
 * Any n_fft is served: L = 80 by the one-tile f32-filter / f64-decision kernel, L >= 160 by streaming chunk sums and a bounded
 * exact search whose LDS footprint does not depend on L (N = 4096 included).
 * How close to the oracle (orc_sc_sync, direct f64 sums per lag): for N = 64 with W = 3 L (k_sc80) and wherever k_sc_tile decides, no
 * decision is taken inside the rounding-error bound of the sums it rests on -- such a lag is summed again as the oracle sums it --, so
 * d_hat is the oracle's at any dynamic range.  The detectors of N >= 128 -- the streaming k_sc_stream and the two-pass k_scb_chunks +
 * k_scb_fine behind it -- decide on slid prefix differences without such a bound: d_hat is the oracle's unless M lies within 1e-12
 * of the threshold (or of the maximum) AND a burst earlier in the capture holds more than 2^9 times the window's energy.  Measured:
 * no difference at a margin of 1e-9 with windows down to 2^-17 of the capture's energy, none at 1e-12 with windows of 2^-9; at 1e-12
 * k_sc_stream differs in 2 of 8 decisions with windows of 2^-15 and in 2 of 8 with 2^-17, k_scb_fine in none of 4 with 2^-15 and in
 * 2 of 4 with 2^-17 (tests/test_gpu_sc_margins.py).  ofdm_params.sync_threshold is a float; the tests set thresholds a float cannot
 * hold through a laboratory key (ofdm_amd/csrc/ofdm_hip_tuning.h). */
int ofdm_sc_correlate_batch(ofdm_ctx *ctx, const ofdm_fc32 *in_dev, int64_t n_frames, int64_t frame_stride,
                            int64_t frame_len, int64_t n_lags, int32_t *d_hat_dev, double *f_delta_dev,
                            float *metric_dev);
/* xcorr_fft (src/signals/mod.rs:186-217) for every capture a[f] (a_len samples) against b (nb samples, device): the full
 * cross-correlation out[i] = sum_n a[n + i - (a_len - 1)] conj(b[n]) over the 2 a_len - 1 fft_shifted indices (zero lag at
 * a_len - 1), idx_max[f] = the FIRST index of the largest |out|^2 (0 when everything is zero, as the reference's loop), peak[f]
 * (optional) = |out[idx_max]|, out_dev (optional, out_stride >= 2 a_len - 1) = the whole output.  Evaluated lag by lag in f64
 * instead of through three odd-length FFTs: the same numbers to ~1e-15.  decode's offset is idx_max - a_len (receiver.rs:21). */
int ofdm_xcorr_batch(ofdm_ctx *ctx, const ofdm_fc32 *a_dev, int64_t n_frames, int64_t a_stride, int64_t a_len,
                     const ofdm_fc32 *b_dev, int32_t nb, int32_t *idx_max_dev, float *peak_dev, ofdm_fc32 *out_dev,
                     int64_t out_stride);
/* frequency_correction (src/receiver.rs:231-240): |mean_m angle(right[m]/left[m])| / L over n_pairs blocks of
 * L = n_fft+cp samples; pair p reads left = in[p*stride ..], right = in[p*stride + right_offset ..] */
int ofdm_frequency_correction_batch(ofdm_ctx *ctx, const ofdm_fc32 *in_dev, int64_t n_pairs, int64_t stride,
                                    int64_t right_offset, double *f_delta_dev);
/* CFO derotation (src/receiver.rs:44-50): x[f][n] *= exp(-j f_delta[f] (first_index[f] + n)), in place.
 * first_index_dev may be NULL (0). */
int ofdm_cfo_rotate_batch(ofdm_ctx *ctx, ofdm_fc32 *x_dev, int64_t n_frames, int64_t frame_stride,
                          int64_t frame_len, const double *f_delta_dev, const int32_t *first_index_dev);
/* estimate_channel (src/receiver.rs:212-229): H[k] = mean_b FFT(block_b minus CP)[k] / training[k] over the five
 * training blocks starting at sample offset_dev[f] + 5*L of frame f (offset_dev NULL: 0).
 * f_delta_dev (optional): blocks are derotated with sample_id counted from offset_dev[f]. hk_dev: n_frames*n_fft
 * Where training[k] = 0 the quotient is 0 / 0: H[k] is non-finite (NaN) in exactly those bins, as the reference's own division
 * leaves it; see ofdm_create for what follows from it.  Under OFDM_CHEST_WLS such a bin has weight 0 and H'[k] is finite. */
int ofdm_estimate_channel_batch(ofdm_ctx *ctx, const ofdm_fc32 *in_dev, int64_t n_frames, int64_t frame_stride,
                                int64_t frame_len, const int32_t *offset_dev, const double *f_delta_dev,
                                ofdm_fc32 *hk_dev);
/* With ofdm_params.chest_mode = OFDM_CHEST_WLS hk_dev receives H' of "channel-estimate denoising" below instead: bit for bit
 * ofdm_chest_smooth_batch of what OFDM_CHEST_LS writes. */

/* ------------------------------------------------------------------ channel-estimate denoising (north-star extension)
 * Parity unpinned by the reference: tests/chest_ref.py is the definition.  With t_k the context's training table, W_k = |t_k|^2 and
 * H^_k the estimate above (so W_k H^_k = conj(t_k) mean_b Y_b[k]; W_k H^_k counts as 0 where t_k = 0):
 *   tap window   L_h = cp_len taps at delays n in [-pre, L_h - pre) taken mod n_fft, pre = cp_len / 4 (a frame start trimmed a few
 *                samples late moves the channel to negative delays; with the default back-off CHANNEL sits at delays 3 .. 13)
 *   estimate     h^ = argmin_h sum_k W_k |H^_k - sum_n h_n e^{-2 pi i k n / N}|^2: maximum likelihood for white noise on the training blocks
 *   closed form  g_n = sum_k W_k H^_k e^{+2 pi i k n / N} (= N IFFT(W o H^) read at the window's indices; the window's offset is only an
 *                index rotation, no phase ramp), h^ = R^-1 g, R[n][m] = r[n - m], r[d] = sum_k W_k e^{+2 pi i k d / N}: Hermitian, Toeplitz,
 *                positive definite, constant per context and independent of pre
 *   output       H'_k = sum_n h^_n e^{-2 pi i k n / N} = FFT of h^ scattered to the window's indices of a zero vector
 * Tables and arithmetic on the device are f32 (k_chest_weight, the generic FFT kernel, k_chest_solve, the generic FFT kernel).
 * A non-finite sample in a training block spoils the frame's WHOLE estimate H', not one bin as with OFDM_CHEST_LS.
 * With chest_mode = OFDM_CHEST_WLS ofdm_estimate_channel_batch returns H' and every decode entry point (ofdm_rx_decode_batch, _host,
 * _long, _long_host, a merged detection included) equalises and forms its LLR weights with H', for every ecc; the fused frame kernels
 * take no estimate from outside, so the generic chain runs (ofdm_last_dispatch shows k_chest_solve).
 * The window and sync_backoff: a Schmidl-Cox frame start lies sync_backoff samples in front of the detected one, which puts the
 * channel's first tap at delay sync_backoff.  The window ends at delay 3 cp_len / 4 - 1, so with sync_backoff >= 3 cp_len / 4 not even
 * a one-tap channel lies inside it and H' is noise: under OFDM_SYNC_SCHMIDL_COX ofdm_create refuses OFDM_CHEST_WLS, and OFDM_CFO_WIDE
 * (whose metric sums the same window), with such a back-off (OFDM_ERR_INVALID).  A channel of T taps needs sync_backoff + T <=
 * 3 cp_len / 4, which is the caller's to keep.  OFDM_SYNC_REFERENCE does not use sync_backoff and takes any. */
/* R^-1 as cp_len x cp_len interleaved (re, im) doubles, row-major, solved in f64 (Levinson recursion + Trench's fill of the Toeplitz
 * inverse, O(cp_len^2)).  training: n_fft interleaved doubles, NULL = the default table.  OFDM_ERR_INVALID for a bad size, a NULL
 * rinv, or a table with so many zero bins that R is singular -- exactly, or to rounding: what the recursion returns is verified,
 * max |R rinv - I| <= 1e-6 over the columns checked (the device keeps the table in f32: beyond that it is no usable table), so a
 * training table that is zero on a whole band (cond(R) 2e14 at n_fft = 256 with the guard bands nulled) is refused, not answered with
 * rounding residue; scattered zero bins leave R well conditioned.  ofdm_create with OFDM_CHEST_WLS and ofdm_chest_smooth_batch refuse
 * the same tables.  Host call, no context: exported so that the solver can be pinned without a GPU. */
int ofdm_chest_matrix(int32_t n_fft, int32_t cp_len, const double *training, double *rinv);
/* The stage on its own: n_frames rows of n_fft bins H^ -> H'.  hk_in_dev == hk_out_dev allowed.  Works on any context whatever its
 * chest_mode (the tables are built on first use; OFDM_ERR_INVALID if the context's training table makes R singular). */
int ofdm_chest_smooth_batch(ofdm_ctx *ctx, const ofdm_fc32 *hk_in_dev, int64_t n_frames, ofdm_fc32 *hk_out_dev);
/* *first_tap = -pre, *n_taps = L_h.  Host call. */
int ofdm_chest_window(const ofdm_ctx *ctx, int32_t *first_tap, int32_t *n_taps);

/* RX demod = unprefix_block + equalise + decode_block + demodulate (src/receiver.rs:64-83) over
 * syms_per_frame OFDM symbols per frame.  Symbol k of frame f starts (at its cyclic prefix) at sample
 * offset_dev[f] + first_symbol*L + k*L of the frame (offset_dev NULL: 0); samples at or beyond frame_len read
 * as zero (pad_chunk, receiver.rs:203-210).  f_delta_dev (optional) derotates with sample_id counted from
 * offset_dev[f].  hk_dev: per-frame channel (hk_stride = n_fft), shared (hk_stride = 0) or NULL (H == 1).
 * out_dev[f*out_stride ..]: syms_per_frame * bytes_per_symbol bytes.  soft_dev (optional): equalised,
 * phase-corrected data points, syms_per_frame*data_carriers per frame. */
int ofdm_rx_demod_batch(ofdm_ctx *ctx, const ofdm_fc32 *in_dev, int64_t n_frames, int64_t frame_stride,
                        int64_t frame_len, int32_t first_symbol, int32_t syms_per_frame,
                        const int32_t *offset_dev, const double *f_delta_dev, const ofdm_fc32 *hk_dev,
                        int64_t hk_stride, uint8_t *out_dev, int64_t out_stride, ofdm_fc32 *soft_dev);

/* ------------------------------------------------------------------ soft decisions (north-star extension)
 * LLR definition, shared by the kernels and tests/soft_ref.py.  A point's bps bits are in demap_point's stream order: the I-axis
 * bits, then the Q-axis bits (BPSK: the I bit only); each axis carries m bits on M = 2^m levels.  With x the equalised,
 * pilot-phase-corrected coordinate, v = x (M - 1) and the levels are the odd integers a_l = 2 l - (M - 1), l in [0, M).  Axis bit b
 * (b = 0 is the Gray MSB) of level l is bit (m - 1 - b) of l ^ (l >> 1), and
 *     Lambda_b(v) = ( min_{l: bit = 0} (v - a_l)^2 - min_{l: bit = 1} (v - a_l)^2 ) / 4          POSITIVE MEANS BIT 1
 * (BPSK / QPSK: Lambda = v, the sign convention of the hard decisions; a noiseless point's weakest bit has |Lambda| = 1).
 * Channel weight w_k = |H_k|^2 / (mean of |H|^2 over the data carriers), per frame or over the shared H; w = 1 without H.
 * Stored: int8 L = clamp(rint(llr_scale * w_k * Lambda), -127, 127), 0 when the product is not finite.  The product is formed in
 * f32: at an llr_scale near FLT_MAX it overflows and 0 is stored where exact arithmetic would clamp to +-127.
 * The true LLR is L / llr_scale * 4 mean|H|^2 / ((M - 1)^2 sigma^2), sigma^2 = the complex noise variance of a received bin:
 * ofdm_rx_quality_batch ("link quality" below) estimates sigma^2 and returns that factor as OFDM_Q_LLR_UNIT.  No decoder scales
 * its LLRs by it; soft combining ("soft combining" below, EXT-7) weighs the captures of one frame by it. */
/* ofdm_rx_demod_batch with int8 LLRs out instead of hard bytes: arguments as there; llr_dev[f*llr_stride ..] receives
 * syms_per_frame * data_carriers * bps LLRs, LLR j = bit j of the stream rx_demod packs LSB-first.  llr_scale must be finite and
 * > 0, llr_stride >= syms_per_frame * data_carriers * bps (OFDM_ERR_INVALID otherwise). */
int ofdm_rx_llr_batch(ofdm_ctx *ctx, const ofdm_fc32 *in_dev, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                      int32_t first_symbol, int32_t syms_per_frame, const int32_t *offset_dev, const double *f_delta_dev,
                      const ofdm_fc32 *hk_dev, int64_t hk_stride, float llr_scale, int8_t *llr_dev, int64_t llr_stride);
/* Soft Hamming(7,4): floor(n_bits / 56) blocks of 8 codewords in ofdm_hamming74_encode's bit layout (7 bits per nibble, low nibble
 * first) -> 4 bytes per block.  Per codeword the c of the 16 that maximises sum_i (2 c_i - 1) L_i, in exact integer arithmetic;
 * ties go to the smallest data nibble. */
int ofdm_hamming74_decode_soft(ofdm_ctx *ctx, const int8_t *llr_dev, int64_t n_bits, uint8_t *out_dev);

/* ------------------------------------------------------------------ link quality (north-star extension)
 * Parity unpinned by the reference, which measures nothing of the kind: tests/quality_ref.py is the definition.  Per frame f, with
 * o = offset_dev[f], S = n_fft + cp_len, samples at or beyond frame_len reading as zero and the derotation of
 * ofdm_estimate_channel_batch (sample id counted from o):
 *   training part, counted only if o >= 0 and o + 10 S <= frame_len (all five training blocks inside the capture):
 *     y_b[n]     the derotated sample o + (5 + b) S + cp_len + n, b < 5, n < n_fft;  ybar = mean_b y_b;  Ybar = FFT(ybar), unnormalised:
 *                the quantity ofdm_estimate_channel_batch divides by the training table
 *     noise_var  (1/4) sum_b sum_n |y_b[n] - ybar[n]|^2  =  (1 / (4 N)) sum_k sum_b |Y_b[k] - Ybar[k]|^2: the unbiased estimate of the
 *                complex noise variance of one received bin, the sigma^2 of "soft decisions" above (formed from the deviations)
 *     gain       sum_{k in D} (|Ybar[k]|^2 - noise_var / 5) / sum_{k in D} |t_k|^2, D = the data carriers, t = the training table:
 *                the |t_k|^2-weighted mean of |H_k|^2 with the noise bias of Ybar removed
 *     snr        max(gain, 0) Es / noise_var, LINEAR (+inf if noise_var is 0); Es = the constellation's mean |point|^2: 1 (BPSK),
 *                2 (QPSK), 2 (M + 1) / (3 (M - 1)) for M levels per axis (10/9, 6/7, 34/45 for 16-, 64-, 256-QAM)
 *     llr_unit   4 mean_{k in D} |hk[f][k]|^2 / ((M - 1)^2 noise_var), M = 2 for BPSK and QPSK, the mean 1 without hk_dev
 *   data part (decision-directed EVM), over the frame's first n_points_dev[f] constellation points in rx_demod's stream order from data
 *   symbol first_symbol (point j lies in symbol j / data_carriers).  Point j is counted iff j < n_points_dev[f], j / data_carriers <
 *   syms_per_frame and its symbol lies wholly inside the capture, o + (first_symbol + j / data_carriers + 1) S <= frame_len:
 *     x          the equalised, pilot-phase-corrected point, what ofdm_rx_demod_batch writes to soft_dev
 *     evm2       sum |x - xh|^2 / sum |xh|^2 over the counted points, xh = the constellation point nearest x (the hard decision mapped
 *                back), LINEAR; 0 when nothing is counted
 *     points     the number counted, as a float
 *   The caller supplies the count because transmit pads the last symbol with zero points, which must not be counted.
 * A frame whose training part is not counted has OFDM_Q_VALID = 0 and every field 0.  A non-finite sample makes the fields it
 * reaches non-finite (one in a training block: noise_var, gain, snr, llr_unit; one in a counted data symbol: evm2); nothing is clamped. */
enum {
    OFDM_Q_VALID = 0,     /* 1 if the training part was counted, else 0 (and the row is 0) */
    OFDM_Q_NOISE_VAR = 1,
    OFDM_Q_GAIN = 2,
    OFDM_Q_SNR = 3,       /* linear */
    OFDM_Q_LLR_UNIT = 4,
    OFDM_Q_EVM2 = 5,      /* linear */
    OFDM_Q_POINTS = 6,
    OFDM_QUALITY_FIELDS = 8 /* floats per row; index 7 is reserved and 0 */
};
/* Arguments as ofdm_rx_demod_batch; quality_dev receives n_frames rows of OFDM_QUALITY_FIELDS floats.  n_points_dev (optional): NULL
 * or a count <= 0 = no EVM.  status_dev (optional): a frame whose status is not OFDM_FRAME_OK gets an all-zero row and is not read.
 * OFDM_ERR_INVALID: NULL in_dev or quality_dev (with n_frames > 0), a negative size, hk_stride not in {0, n_fft}, or syms_per_frame *
 * data_carriers above 2^24 (points is a float: no frame may count more; a larger n_points_dev[f] counts what syms_per_frame holds).
 * n_frames == 0: OFDM_OK.  One launch (k_linkq), no workspace. */
int ofdm_rx_quality_batch(ofdm_ctx *ctx, const ofdm_fc32 *in_dev, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                          int32_t first_symbol, int32_t syms_per_frame, const int32_t *n_points_dev,
                          const int32_t *offset_dev, const double *f_delta_dev, const ofdm_fc32 *hk_dev, int64_t hk_stride,
                          const int32_t *status_dev, float *quality_dev);

/* ------------------------------------------------------------------ wide CFO acquisition (north-star extension)
 * The Schmidl-Cox phase gives the carrier offset modulo 2 pi / S rad/sample, S = n_fft + cp_len: an acquisition range of +-pi / S,
 * +-0.4 sub-carrier spacings.  A capture whose offset is f0 + 2 pi m / S with m != 0 is detected with a perfect timing metric, derotated
 * by f0 alone and demodulated into garbage.  The frame already carries what resolves m: the five training blocks are identical and one
 * symbol long, so a hypothesis m rotates every block alike, and for the right m their sum, matched against the known training table,
 * puts its energy into the cp_len delays a channel can occupy; for a wrong m the energy spreads over all n_fft delays.
 * Parity unpinned by the reference (its frequency_correction has the same ambiguity and drops the sign as well): tests/cfo_wide_ref.py
 * is the definition.  Per frame f, with o = offset_dev[f], f0 = f_delta_dev[f] on entry, N = n_fft, cp = cp_len, samples at or beyond
 * frame_len reading as zero and the derotation of ofdm_estimate_channel_batch (sample id counted from o):
 *   tested     iff status_dev[f] == 0 (or no status_dev), o >= 0 and o + 10 S <= frame_len (all five training blocks inside the capture);
 *              a frame that is not tested gets m = 0 and both metrics 0, and its f_delta is untouched
 *   ybar[n]    sum_{b < 5} x[o + (5 + b) S + cp + n] e^{-i f0 ((5 + b) S + cp + n)}, n < N: the SUM ofdm_estimate_channel_batch forms
 *   z_m[n]     ybar[n] e^{-2 pi i m (cp + n) / S}
 *   g_m        IFFT_N(conj(t) o FFT_N(z_m)), t = the context's training table.  Scaling: the forward transform unnormalised, the inverse
 *              one carrying the 1 / N, ybar the sum (not the mean) of the blocks
 *   G_m        sum of |g_m[n]|^2 over the delays n in [-pre, L_h - pre) mod N, L_h = cp_len, pre = cp_len / 4: ofdm_chest_window's
 *   decision   the hypotheses are visited in the order 0, -1, +1, -2, +2, ..., -span, +span; one is kept only if its G is strictly
 *              greater than the best so far.  m = the kept one, metric[0] = G_m, metric[1] = the largest G among the others
 *   result     f_delta_dev[f] = f0 + 2 pi m / S, formed in f64; for m = 0 the value is f0 bit for bit
 * A non-finite sample in a training block gives m = 0 and non-finite metrics, in that frame only.  Arithmetic on the device is f32 (the
 * phases are reduced in f64); measured over the oracle's frames the winner's G is at least twice the runner-up's wherever Schmidl-Cox
 * detects the frame at all, so the f32 decision is the f64 one.
 * cfo_mode = OFDM_CFO_WIDE: every decode entry point (ofdm_rx_decode_batch, _host, _long, _long_host, _combine_batch) runs the stage
 * with span = OFDM_CFO_WIDE_SPAN directly behind the Schmidl-Cox search, for every ecc and chest_mode; everything behind it derotates
 * with the total offset, and the f_delta it returns is the total offset: +-(OFDM_CFO_WIDE_SPAN + 0.5) 2 pi / S, +-6.8 sub-carrier
 * spacings instead of +-0.4.  ofdm_last_dispatch shows k_cfo_wide behind k_rx_prepare. */
/* The stage on its own, on any context whatever its cfo_mode.  1 <= span <= OFDM_CFO_WIDE_MAX_SPAN.  status_dev, m_dev and metric_dev
 * (2 floats per frame) are optional.  OFDM_ERR_INVALID: a NULL context, NULL in_dev, offset_dev or f_delta_dev (with n_frames > 0), a
 * negative size, frame_len <= 0 or a span outside its range.  n_frames == 0: OFDM_OK.  One launch (k_cfo_wide), no workspace. */
int ofdm_cfo_wide_batch(ofdm_ctx *ctx, const ofdm_fc32 *in_dev, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                        const int32_t *offset_dev, const int32_t *status_dev /* optional */, int32_t span,
                        double *f_delta_dev /* in: f0, out: f0 + 2 pi m / S */, int32_t *m_dev /* optional */,
                        float *metric_dev /* optional, 2 per frame */);

/* ------------------------------------------------------------------ noise-aware LLR weights (EXT-11) (north-star extension)
 * The channel weight w_k of "soft decisions" above assumes the same noise on every carrier.  A narrow-band interferer, an LO spur or a
 * DC offset puts a few carriers far under the rest, and those then hand the decoder confident wrong LLRs.  The five training blocks are
 * identical, so their scatter is the noise; "link quality" sums it over all bins into one noise_var, here it is kept per bin.
 * Parity unpinned by the reference, which has nothing of the kind: tests/noise_weight_ref.py is the definition.  Per frame f, with
 * o = offset_dev[f], S = n_fft + cp_len, N = n_fft, samples at or beyond frame_len reading as zero and the derotation of
 * ofdm_estimate_channel_batch (sample id counted from o):
 *   tested     iff status_dev[f] == 0 (or no status_dev), o >= 0 and o + 10 S <= frame_len (all five training blocks inside the capture);
 *              a frame that is not tested is not read and gets s_k = 0 and q_k = 1 for every k
 *   y_b[n]     the derotated sample o + (5 + b) S + cp_len + n, b < 5, n < N, as "link quality" forms it;  ybar = mean_b y_b;
 *              d_b = y_b - ybar, formed in the time domain, before any transform, as (1/5) sum_c (y_b - y_c): five identical blocks
 *              give exactly 0
 *   s_k        (1/4) sum_b |FFT_N(d_b)[k]|^2, the transform unnormalised: the unbiased estimate of the complex noise variance of
 *              received bin k.  The mean of s_k over all N bins is OFDM_Q_NOISE_VAR.
 *   sbar       the mean of s_k over all N bins
 *   q_k        sbar / s_k if s_k > sbar, else 1 (the comparison is false for NaN).  0 <= q_k <= 1; a noiseless frame has q = 1 everywhere.
 *              The estimate has four degrees of freedom per bin, which is why it may only lower a carrier's weight, never raise it.
 *   LLR        L = clamp(rint(((llr_scale nd / sum |H|^2) |H_k|^2) q_k Lambda), -127, 127), the f32 products formed in that order
 *              (the scale of ofdm_rx_llr_batch, one more multiply, then Lambda); 0 when the product is not finite.  Hard decisions,
 *              equalisation and pilot phase are those of ofdm_rx_llr_batch.
 * q is homogeneous of degree 0 in the capture and s of degree 2: under a gain +-2^k, q keeps its bits and s is scaled by 4^k exactly.
 * What the scatter cannot see: an interferer whose phase advances a whole number of turns per symbol (a tone at bin x with x S / N an
 * integer) is the same in all five blocks and counts as signal; and a tone within ~5 dB of the frame's own power hits the timing
 * search, the pilots and the channel estimate, which this feature leaves as they are. */
enum { OFDM_LLRW_CHANNEL = 0, /* w_k alone: the default, bit for bit what the library did before the mode existed */
       OFDM_LLRW_NOISE = 1    /* w_k q_k */ };
/* The estimate on its own.  nvar_dev (optional) receives n_frames rows of n_fft floats s_k, weight_dev (optional) as many q_k; bin k of
 * frame f is element f * n_fft + k.  status_dev and f_delta_dev (NULL: no derotation) are optional.  OFDM_ERR_INVALID: a NULL context,
 * NULL in_dev or offset_dev (with n_frames > 0), a negative size or frame_len <= 0.  n_frames == 0: OFDM_OK.  One launch
 * (k_noise_bins), no workspace; the rows' bits do not depend on the grid. */
int ofdm_rx_noise_bins_batch(ofdm_ctx *ctx, const ofdm_fc32 *in_dev, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                             const int32_t *offset_dev, const double *f_delta_dev, const int32_t *status_dev /* optional */,
                             float *nvar_dev /* optional, n_frames * n_fft */, float *weight_dev /* optional, n_frames * n_fft */);
/* ofdm_rx_llr_batch with the LLR scale of bin k multiplied by bin_weight_dev[f * bin_weight_stride + k] (k_sym<llrw>): arguments and
 * checks as there; bin_weight_stride must be 0 (one row of n_fft floats shared by every frame) or n_fft (OFDM_ERR_INVALID otherwise).
 * The weights are taken as they are: nothing holds them to [0, 1].  bin_weight_dev == NULL is ofdm_rx_llr_batch itself: the same
 * kernel, the same bytes. */
int ofdm_rx_llr_weighted_batch(ofdm_ctx *ctx, const ofdm_fc32 *in_dev, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                               int32_t first_symbol, int32_t syms_per_frame, const int32_t *offset_dev, const double *f_delta_dev,
                               const ofdm_fc32 *hk_dev, int64_t hk_stride, float llr_scale, int8_t *llr_dev, int64_t llr_stride,
                               const float *bin_weight_dev, int64_t bin_weight_stride);
/* The mode of a context: OFDM_LLRW_CHANNEL (the default) or OFDM_LLRW_NOISE; any other value is OFDM_ERR_INVALID and changes nothing.
 * It is not part of ofdm_params.  Under OFDM_LLRW_NOISE every decode entry point that forms LLRs (ofdm_rx_decode_batch, _host, _long,
 * _long_host, their sc16 forms and ofdm_rx_decode_combine_batch, for every soft ecc, chest_mode and cfo_mode) runs k_noise_bins behind
 * the channel estimate, over the chain's own offset, f_delta and status, into a workspace of the context, and k_sym<llrw> in place of
 * k_sym<llr>: the chain is the composition of ofdm_rx_noise_bins_batch, ofdm_rx_llr_weighted_batch and the mode's decoder, bit for bit,
 * and ofdm_last_dispatch shows both kernels.  A mode that forms no LLRs (ecc 0, 1, 20, 64, 65, 84) is untouched: the same kernels, the
 * same bytes.  The link-quality rows and the combine weights of ofdm_rx_decode_combine_batch do not change with the mode.  The rule
 * costs a little in a clean channel near the decoder's waterfall, which is why it is opt-in. */
int ofdm_set_llr_weight(ofdm_ctx *ctx, int32_t mode);
int ofdm_get_llr_weight(const ofdm_ctx *ctx, int32_t *mode);

/* ------------------------------------------------------------------ convolutional code (north-star extension; DESIGN.md 3, EXT-2 convolutional code)
 * K = 7, rate 1/2, generators 133 / 171 octal; the definition shared by the kernels and tests/conv_ref.py.
 * Encoder: input bits u_t, t in [0, T): the payload bytes followed by ONE 0x00 tail byte, each byte LSB first, T = 8 (p + 1).
 * Register r_t = (u_t << 6) | s_t, state s_t = the previous six inputs (u_{t-1} at bit 5 .. u_{t-6} at bit 0), s_0 = 0;
 * A_t = parity(r_t & 0133), B_t = parity(r_t & 0171), s_{t+1} = r_t >> 1.  Coded stream c_{2t} = A_t, c_{2t+1} = B_t, packed LSB
 * first: 2 (p + 1) bytes, no padding bits.  The tail byte returns the encoder to state 0.
 * Decoder: int8 LLRs L_j, positive = bit 1, L_{2t} for A_t, L_{2t+1} for B_t.  Path metrics are maximised in exact int32 arithmetic:
 * PM_0[0] = 0, every other state excluded at t = 0.  State s' at t + 1 has input u = s' >> 5 and predecessors p0 = (s' & 31) << 1,
 * p1 = p0 | 1; a transition with outputs (a, b) adds (2a - 1) L_{2t} + (2b - 1) L_{2t+1}; the survivor is p1 iff its candidate is
 * strictly larger (a tie keeps p0).  Traceback starts at state 0 when `terminated`, otherwise at the largest final metric (lowest
 * state on a tie); u_t = s_{t+1} >> 5, output bytes packed LSB first.  That is maximum likelihood over all T-bit inputs (whose last
 * six bits are zero when terminated).  Puncturing: see "punctured rates and framed modes" below.  No interleaver, no sliding window:
 * the whole frame is traced back. */
/* rows of n_bytes payload bytes -> rows of 2 * (n_bytes + 1) coded bytes (row f at in_dev + f * in_stride / out_dev + f * out_stride;
 * in_stride >= n_bytes, out_stride >= 2 * (n_bytes + 1), OFDM_ERR_INVALID otherwise) */
int ofdm_conv_k7_encode(ofdm_ctx *ctx, const uint8_t *in_dev, int64_t n_frames, int64_t in_stride, int64_t n_bytes,
                        uint8_t *out_dev, int64_t out_stride);
/* rows of 2 * n_steps LLRs -> rows of floor(n_steps / 8) bytes (a tail byte, if the caller coded one, included).  llr_stride >=
 * 2 * n_steps, out_stride >= floor(n_steps / 8) (OFDM_ERR_INVALID otherwise); n_steps > 2^20: OFDM_ERR_UNSUPPORTED (the int32 path
 * metrics are not renormalised).  n_steps = 0 and n_frames = 0 succeed and write nothing. */
int ofdm_conv_k7_decode_soft(ofdm_ctx *ctx, const int8_t *llr_dev, int64_t n_frames, int64_t llr_stride, int64_t n_steps,
                             int32_t terminated, uint8_t *out_dev, int64_t out_stride);

/* ------------------------------------------------------------------ punctured rates and framed modes (DESIGN.md 3, EXT-2 framed modes)
 * Parity unpinned by the reference: tests/framed_ref.py is the definition.
 * Rates.  A keep mask, periodic in the step index t, lists (A_t, B_t): rate 1/2 (1,1); rate 2/3 (1,1),(1,0); rate 3/4
 * (1,1),(1,0),(0,1) -- the 802.11a patterns.  kept(T, rate) = the ones of the mask over steps 0 .. T - 1.  The punctured stream is the
 * kept bits of c_0, c_1, ... of the encoder above, in order, packed LSB first and zero-padded to a whole byte:
 * ceil(kept(8 (p + 1), rate) / 8) bytes for p payload bytes and the tail byte.  The decoder puts LLR 0 at every dropped position and
 * then runs exactly the Viterbi rule above (same tie rules, same `terminated`).
 * Framed modes (ecc = OFDM_ECC_CONV_K7F_R12 / _R23 / _R34).  Behind its usual 16-byte header a frame carries
 *   1. the length block, always rate 1/2: the code above over the 8 bytes [u32 LE p][u32 LE ~p] and the tail byte = 18 bytes, 72 steps;
 *   2. the body: the payload's p bytes and the tail byte at the mode's rate.
 * coded_len(p) = 18 + ceil(kept(8 (p + 1), rate) / 8); the 16-byte header carries coded_len of the row's true length as in every
 * mode, and the frame is the OFDM_ECC_NONE frame of that byte stream.  With per-row lengths row f codes its own len_f into both blocks.
 * Decode of a frame that reached the demodulator (status OFDM_FRAME_OK so far), body = the demodulated bytes behind the 16-byte header,
 * which is NOT read: body < 18 -> status OFDM_FRAME_HEADER, out_len 0.  Otherwise 72 steps, terminated, are decoded from LLRs 128 ..
 * 272; the block is valid iff bytes 4..7 are the complement of bytes 0..3 and byte 8 is 0, an invalid one gives OFDM_FRAME_HEADER and
 * out_len 0 (a garbled length is reported, never guessed).  With a valid p and avail = body - 18: if ceil(kept(8 (p + 1)) / 8) <=
 * avail, 8 (p + 1) steps are decoded, terminated, from LLR 272 on and p bytes delivered; otherwise the frame was cut short: the
 * largest T' with kept(T') <= 8 avail steps are decoded unterminated, min(p, T' / 8) bytes delivered, status unchanged. */
/* kept(n_steps, rate); host call, no context.  OFDM_ERR_INVALID (< 0) for a rate that is not OFDM_CONV_RATE_* or n_steps < 0 */
int64_t ofdm_conv_k7_kept_bits(int64_t n_steps, int32_t rate);
/* ofdm_conv_k7_encode at `rate`: rows of n_bytes payload bytes -> rows of ceil(kept(8 (n_bytes + 1), rate) / 8) bytes; in_stride >=
 * n_bytes, out_stride >= that row (OFDM_ERR_INVALID otherwise, and for an unknown rate).  rate = OFDM_CONV_RATE_1_2: the bytes of
 * ofdm_conv_k7_encode. */
int ofdm_conv_k7_encode_punctured(ofdm_ctx *ctx, const uint8_t *in_dev, int64_t n_frames, int64_t in_stride, int64_t n_bytes,
                                  int32_t rate, uint8_t *out_dev, int64_t out_stride);
/* ofdm_conv_k7_decode_soft at `rate`: rows of kept(n_steps, rate) LLRs (the kept positions only) -> rows of floor(n_steps / 8) bytes.
 * llr_stride >= kept(n_steps, rate), out_stride >= floor(n_steps / 8) (OFDM_ERR_INVALID otherwise); n_steps > 2^20:
 * OFDM_ERR_UNSUPPORTED.  rate = OFDM_CONV_RATE_1_2: the bytes of ofdm_conv_k7_decode_soft. */
int ofdm_conv_k7_decode_punctured(ofdm_ctx *ctx, const int8_t *llr_dev, int64_t n_frames, int64_t llr_stride, int64_t n_steps,
                                  int32_t rate, int32_t terminated, uint8_t *out_dev, int64_t out_stride);

/* ------------------------------------------------------------------ outer Reed-Solomon code on the device (DESIGN.md 3, EXT-2 RS outer code)
 * The code of ofdm_rs255_encode / ofdm_rs255_decode above, batched on device buffers on the context's stream (k_rs255_encode /
 * k_rs255_decode).  Definition of a block's decode: the unique code word within 16 byte errors of the received 255 bytes if there is
 * one, failure otherwise -- a function of the received bytes alone, also beyond 16 errors (the decoder checks that what it corrected
 * is a code word).  The host functions are the executable form, and the device agrees with them on every input.
 * encode: row f = in_dev[f*in_stride .. + len_f), len_f = in_len_dev[f] clamped to [0, n_bytes], or n_bytes when NULL, is coded as
 *   ofdm_rs255_encode codes it into out_dev[f*out_stride ..]: 255 (len_f / 223 + 1) bytes; the bytes behind them, up to
 *   ofdm_rs255_encoded_len(n_bytes), are written as 0.  in_stride >= n_bytes, out_stride >= ofdm_rs255_encoded_len(n_bytes).
 * decode: row f = code_dev[f*code_stride .. + len_f), len_f = code_len_dev[f] clamped to [0, n_code], or n_code when NULL, is cut
 *   into 255-byte blocks, the zero-padded remainder included even if it is empty, and 223 (len_f / 255 + 1) bytes are written to
 *   out_dev[f*out_stride ..]; out_len_dev[f] (optional) = that count.  corrected_dev[f] (optional) = corrected bytes of the row, or
 *   -1 if a block of the row cannot be decoded: the row is still written in full, decodable blocks corrected, the 223 data bytes of an
 *   undecodable block as received, and the call returns OFDM_OK (OFDM_ERR_UNCORRECTABLE stays the host function's code).
 *   code_stride >= n_code, out_stride >= ofdm_rs255_decoded_len(n_code).
 * A violated stride rule, a negative count or a NULL context: OFDM_ERR_INVALID.  n_frames == 0: OFDM_OK, nothing is written.
 *
 * Frame modes ecc = OFDM_ECC_RS255* = 20 + inner.  Transmit: the frame is the inner mode's frame of ofdm_rs255_encode(payload), so
 * coded_len(p) = inner_coded_len(255 (p / 223 + 1)); with per-row lengths row f codes its own len_f.  Receive: the inner mode's chain
 * runs unchanged; a frame whose status it leaves at OFDM_FRAME_OK with len bytes is decoded as ofdm_rs255_decode decodes those len
 * bytes: out_len = 223 (len / 255 + 1) -- the payload, zero-padded to whole blocks, trailing zero block included, as
 * decipher_transmission_bytes returns it -- or, if a block cannot be decoded, status OFDM_FRAME_UNCORRECTABLE and out_len 0 (the
 * reference returns None).  A frame with any other inner status keeps it, with out_len 0.  Rows: out_stride >= 223 (Lmax / 255 + 1),
 * Lmax = the row size the inner mode asks for the same max_symbols (OFDM_ERR_INVALID otherwise), in every decode entry point. */
int ofdm_rs255_encode_batch(ofdm_ctx *ctx, const uint8_t *in_dev, int64_t n_frames, int64_t in_stride, const int32_t *in_len_dev,
                            int64_t n_bytes, uint8_t *out_dev, int64_t out_stride);
int ofdm_rs255_decode_batch(ofdm_ctx *ctx, const uint8_t *code_dev, int64_t n_frames, int64_t code_stride, const int32_t *code_len_dev,
                            int64_t n_code, uint8_t *out_dev, int64_t out_stride, int32_t *out_len_dev, int32_t *corrected_dev);

/* ------------------------------------------------------------------ LDPC(648,324) (north-star extension; DESIGN.md 3, EXT-2 LDPC)
 * Parity unpinned by the reference (it has no LDPC code): tests/ldpc_ref.py (numpy, exact integers) is the definition;
 * ofdm_ldpc648_encode / ofdm_ldpc648_decode are its executable form on the host, and the device agrees with both bit for bit.
 * The code: quasi-cyclic, Z = 27, 12 x 24 blocks, 88 of them non-zero; entry s is the 27 x 27 identity shifted so that check z of block
 * row l touches variable 27 c + (z + s) mod 27 of block column c, "-" a zero block:
 *      0  -  -  -  0  0  -  -  0  -  -  0  1  0  -  -  -  -  -  -  -  -  -  -
 *     22  0  -  - 17  -  0  0 12  -  -  -  -  0  0  -  -  -  -  -  -  -  -  -
 *      6  -  0  - 10  -  -  - 24  -  0  -  -  -  0  0  -  -  -  -  -  -  -  -
 *      2  -  -  0 20  -  -  - 25  0  -  -  -  -  -  0  0  -  -  -  -  -  -  -
 *     23  -  -  -  3  -  -  -  0  -  9 11  -  -  -  -  0  0  -  -  -  -  -  -
 *     24  - 23  1 17  -  3  - 10  -  -  -  -  -  -  -  -  0  0  -  -  -  -  -
 *     25  -  -  -  8  -  -  -  7 18  -  -  0  -  -  -  -  -  0  0  -  -  -  -
 *     13 24  -  -  0  -  8  -  6  -  -  -  -  -  -  -  -  -  -  0  0  -  -  -
 *      7 20  - 16 22 10  -  - 23  -  -  -  -  -  -  -  -  -  -  -  0  0  -  -
 *     11  -  -  - 19  -  -  - 13  -  3 17  -  -  -  -  -  -  -  -  -  0  0  -
 *     25  -  8  - 23 18  - 14  9  -  -  -  -  -  -  -  -  -  -  -  -  -  0  0
 *      3  -  -  - 16  -  -  2 25  5  -  -  1  -  -  -  -  -  -  -  -  -  -  0
 * It is intended to be the n = 648, rate-1/2 matrix of 802.11n, written from memory and UNVERIFIED against the standard; this table
 * is the definition (rank 324, invertible parity half, no 4-cycles: tests/test_ldpc_cpu.py).
 * Code word: x[0 .. 319] = the 40 info bytes, each LSB first; x[320 .. 323] = 0 (shortened); x[324 .. 647] = the unique parity with
 * H x = 0.  Sent: x[0 .. 319] ++ x[324 .. 643] packed LSB first, 80 bytes; the last four parity bits are punctured.
 * Decoder: 640 int8 LLRs a code word, positive = bit 1.  Layered normalised min-sum, factor 3/4, exact integers; inside, positive =
 * bit 0.  Q_v = -L_v (v < 320), +2047 (v = 320 .. 323), -L_{v-4} (v = 324 .. 643), 0 (v = 644 .. 647); all R = 0.  Iterations it =
 * 1, 2, ...; in each the block rows l = 0 .. 11 in order; for check z of the row, with its edges e in table order and v_e their
 * variables:  T_e = clamp(Q_{v_e} - R_e, +-2047);  m_e = min over e' != e of |T_e'|;  sign_e = product over e' != e of (T_e' < 0 ? -1
 * : +1);  R_e = sign_e min((3 m_e) >> 2, 127);  Q_{v_e} = clamp(T_e + R_e, +-2047).  After each whole iteration x_v = (Q_v < 0): if
 * all 324 checks hold the code word has CONVERGED at iteration it and stops; otherwise up to max_iter iterations run.  The output is
 * always x[0 .. 319] of the last iteration run; iters = it when converged, 0 when not.
 * ofdm_ldpc648_coded_len(p) = 80 ceil((p + 8) / 40) (OFDM_ERR_INVALID for p < 0): host call, no context.
 * ofdm_ldpc648_encode: n_cw blocks of 40 info bytes -> n_cw blocks of 80 code bytes, on the host.
 * ofdm_ldpc648_decode: n_cw blocks of 640 LLRs -> n_cw blocks of 40 bytes and iters[n_cw] (optional), on the host; max_iter in 1 .. 64.
 * ofdm_ldpc648_encode_batch / _decode_batch (k_ldpc_encode / k_ldpc_decode): the same on device rows, row f holding n_cw plain code
 *   words (no frame rule); every code word runs to convergence or max_iter; iters_dev (optional) holds n_frames * n_cw counts, row
 *   after row.  in_stride >= 40 n_cw and out_stride >= 80 n_cw (encode), llr_stride >= 640 n_cw and out_stride >= 40 n_cw (decode),
 *   max_iter in 1 .. 64, n_frames, n_cw >= 0: OFDM_ERR_INVALID otherwise.  A zero count succeeds and writes nothing.
 *
 * Frame mode ecc = OFDM_ECC_LDPC648.  Info stream of a payload of p bytes: [u32 LE p][u32 LE ~p] ++ payload, zero-padded to B =
 * ceil((p + 8) / 40) code words; coded_len(p) = 80 B; the frame is the OFDM_ECC_NONE frame of the coded stream (its 16-byte header
 * carries 80 B and decode does not read it).  With per-row lengths row f codes its own len_f, zeros behind.
 * Receive, for a frame the chain leaves at OFDM_FRAME_OK, body = the demodulated bytes behind the 16-byte header, nb = body / 80:
 *   nb = 0: status OFDM_FRAME_HEADER, out_len 0.  Code word 0 is decoded from LLRs 128 .. 767 (OFDM_SOFT_LLR_SCALE, OFDM_LDPC_MAX_ITER
 *   iterations at most); unconverged, or its bytes 4 .. 7 not the complement of bytes 0 .. 3: OFDM_FRAME_HEADER, out_len 0.  With p =
 *   bytes 0 .. 3 and B = ceil((p + 8) / 40), computed in 64 bits, code words 1 .. min(B, nb) - 1 are decoded; one unconverged:
 *   OFDM_FRAME_UNCORRECTABLE, out_len 0.  Otherwise min(p, 40 nb - 8) bytes are delivered with the status unchanged: a frame cut by
 *   the end of the capture delivers its prefix.  Bytes of a row beyond out_len are unspecified.
 * Rows: out_stride >= max(40 floor(body_max / 80) - 8, 0), body_max = max(max_symbols * bytes_per_symbol - 16, 0) (OFDM_ERR_INVALID
 * otherwise), in every decode entry point (ofdm_rx_decode_batch, _host, _long, _long_host); chest_mode is honoured.  OFDM_ECC_FCS +
 * OFDM_ECC_LDPC648 wraps the mode like any other; 20 + 16 (RS outside LDPC) is rejected.
 *
 * LDPC(648), rates 2/3, 3/4 and 5/6 (OFDM_ECC_LDPC648_R23 / _R34 / _R56; tests/ldpc_rates_ref.py is the definition, for rate 1/2 it is
 * ldpc_ref.py again).  `rate`: 0 = 1/2 (the code above), 1 = 2/3, 2 = 3/4, 3 = 5/6; every other value OFDM_ERR_INVALID.  All four are
 * quasi-cyclic with Z = 27 and 24 block columns, 12 / 8 / 6 / 4 block rows, and the entry convention and the parity structure of the
 * table above: the first parity column carries shifts 1 / 0 / 1 in the first, the middle (rows / 2) and the last block row, then the
 * dual diagonal.  The three tables below are THE PROJECT'S OWN, found by a seeded greedy search (row degrees balanced, no 4-cycles, the
 * fewest 6-cycles of 30 draws); they are NOT the matrices of 802.11n.  The tables are the definition (full rank 216 / 162 / 108,
 * invertible parity halves, no 4-cycles: tests/test_ldpc_rates_cpu.py).
 *   rate 2/3, 8 x 24, 87 blocks:
 *     15  5 24  -  3 14  -  -  8 23  -  4  -  - 13  -  1  0  -  -  -  -  -  -
 *      5  2 12  9  - 17  -  1  -  - 10  - 26  -  -  -  -  0  0  -  -  -  -  -
 *     21 24 22  2  -  2 25  -  4  -  -  5  -  -  -  -  -  -  0  0  -  -  -  -
 *     26 13  7 22  -  - 15  - 11  - 18  - 17  -  -  4  -  -  -  0  0  -  -  -
 *      0  5  - 15  0 24  - 11  - 10  -  -  -  0  1  -  0  -  -  -  0  0  -  -
 *      3 21 18 12 22  - 25  -  - 22  -  - 16  -  -  5  -  -  -  -  -  0  0  -
 *      5 14 22  8  -  - 13 14  -  - 18  -  -  2  - 11  -  -  -  -  -  -  0  0
 *      4 17  7  5 26  -  -  3  -  -  -  5  -  8 16  -  1  -  -  -  -  -  -  0
 *   rate 3/4, 6 x 24, 85 blocks:
 *     11 13 17 14 16  - 14 20  - 26  -  2 26  -  - 26 23  -  1  0  -  -  -  -
 *     21  3 11 15 13 26  5  -  - 15  -  8  - 13  - 21  - 18  -  0  0  -  -  -
 *     22  1 21  6 21  8  - 20 25  - 16  -  9  -  - 17  - 25  -  -  0  0  -  -
 *     18 22 11 25 18 13  - 13 26  - 22  - 21  - 16  -  4  -  0  -  -  0  0  -
 *     13 18  5 12 20  -  3 21  0  -  - 11  - 25  8  - 19  -  -  -  -  -  0  0
 *     25 22 21  3 13 24 10  -  - 24 12  -  -  3 10  -  -  3  1  -  -  -  -  0
 *   rate 5/6, 4 x 24, 81 blocks:
 *     10 13 21 20 13 19 12 15  6 26 10 20  9  - 11 18  - 10 19 23  1  0  -  -
 *      5 21 26 18 17 12 15 14  2 18  0  9  - 23 20 20 21  -  4  7  -  0  0  -
 *     19 20  4 22 11  7 13 11 14 20 16 17 22 15  0  - 14 10  - 13  0  -  0  0
 *     22 15 22 11 21  3 21 25 12 19  8 23  8 22  - 23 19  4  6  -  1  -  -  0
 * Every rate sends 640 bits = 80 bytes a code word.  With M = 27 rows checks and K = ofdm_ldpc648_info_bytes(rate) = 40 / 53 / 60 / 67:
 * x[0 .. 8 K - 1] = the K info bytes, LSB first; x[8 K .. 647 - M] = 0 (shortened: 4 / 8 / 6 / 4 bits, not sent); x[648 - M .. 647] =
 * the unique parity with H x = 0.  Sent: x[0 .. 8 K - 1] ++ x[648 - M .. 648 - M + (640 - 8 K) - 1], packed LSB first: 320 of 324 /
 * all 216 / 160 of 162 / 104 of 108 parity bits, the last 4 / 0 / 2 / 4 are punctured.  The decoder is the one above over the code's
 * table: shortened positions start at +2047, punctured ones at 0, sent ones at -L; output x[0 .. 8 K - 1].
 * ofdm_ldpc648_info_bytes(rate) = K.  ofdm_ldpc648_coded_len_rate(p, rate) = 80 ceil((p + 8) / K).
 * ofdm_ldpc648_encode_rate / _decode_rate: n_cw blocks of K info bytes -> n_cw blocks of 80 code bytes, and n_cw blocks of 640 LLRs ->
 *   n_cw blocks of K bytes and iters[n_cw] (optional), on the host.  ofdm_ldpc648_encode_rate_batch / _decode_rate_batch
 *   (k_ldpc_encode<r23|r34|r56> / k_ldpc_decode<r23|r34|r56>; rate 0: k_ldpc_encode / k_ldpc_decode): the same on device rows, with
 *   in_stride >= K n_cw and out_stride >= 80 n_cw (encode), llr_stride >= 640 n_cw and out_stride >= K n_cw (decode).  Rate 0 through
 *   any of them gives what the functions without `rate` give, byte for byte.
 * Frame modes ecc = OFDM_ECC_LDPC648_R23 / _R34 / _R56: the frame rule of OFDM_ECC_LDPC648 above with K in place of 40 -- info stream
 * [u32 LE p][u32 LE ~p] ++ payload, zero-padded to B = ceil((p + 8) / K) code words, coded_len(p) = 80 B; receive with nb = body / 80:
 * the same OFDM_FRAME_HEADER / OFDM_FRAME_UNCORRECTABLE verdicts, min(p, K nb - 8) bytes delivered; rows: out_stride >= max(K
 * floor(body_max / 80) - 8, 0).  OFDM_ECC_FCS + each wraps it like any other mode; 20 + each (61 .. 63) is rejected. */
int64_t ofdm_ldpc648_coded_len(int64_t payload_bytes);
int ofdm_ldpc648_encode(const uint8_t *info, int64_t n_cw, uint8_t *code);
int ofdm_ldpc648_decode(const int8_t *llr, int64_t n_cw, int32_t max_iter, uint8_t *out, int32_t *iters);
int ofdm_ldpc648_encode_batch(ofdm_ctx *ctx, const uint8_t *in_dev, int64_t n_frames, int64_t in_stride, int64_t n_cw, uint8_t *out_dev,
                              int64_t out_stride);
int ofdm_ldpc648_decode_batch(ofdm_ctx *ctx, const int8_t *llr_dev, int64_t n_frames, int64_t llr_stride, int64_t n_cw, int32_t max_iter,
                              uint8_t *out_dev, int64_t out_stride, int32_t *iters_dev /* optional, n_frames * n_cw */);
int32_t ofdm_ldpc648_info_bytes(int32_t rate);
int64_t ofdm_ldpc648_coded_len_rate(int64_t payload_bytes, int32_t rate);
int ofdm_ldpc648_encode_rate(const uint8_t *info, int64_t n_cw, int32_t rate, uint8_t *code);
int ofdm_ldpc648_decode_rate(const int8_t *llr, int64_t n_cw, int32_t max_iter, int32_t rate, uint8_t *out, int32_t *iters);
int ofdm_ldpc648_encode_rate_batch(ofdm_ctx *ctx, const uint8_t *in_dev, int64_t n_frames, int64_t in_stride, int64_t n_cw, int32_t rate,
                                   uint8_t *out_dev, int64_t out_stride);
int ofdm_ldpc648_decode_rate_batch(ofdm_ctx *ctx, const int8_t *llr_dev, int64_t n_frames, int64_t llr_stride, int64_t n_cw, int32_t max_iter,
                                   int32_t rate, uint8_t *out_dev, int64_t out_stride, int32_t *iters_dev /* optional, n_frames * n_cw */);

/* ------------------------------------------------------------------ frame check sequence (north-star extension; DESIGN.md 3, EXT-2 frame check)
 * Parity unpinned by the reference (it has no check of its own): tests/fcs_ref.py over zlib.crc32 is the definition.
 * crc32 = the CRC of IEEE 802.3 / zlib: reflected polynomial 0xEDB88320, register initialised to 0xFFFFFFFF, result complemented;
 * crc32("123456789") = 0xCBF43926.
 * Envelope of a payload of p bytes, p + OFDM_FCS_OVERHEAD bytes long:
 *     E(payload) = [u32 LE p] ++ payload ++ [u32 LE crc32([u32 LE p] ++ payload)]
 * Check of a delivered row of L bytes: valid iff L >= 8, p = the u32 at byte 0 satisfies p <= L - 8 (compared in 64 bits: p may be
 * 0xFFFFFFFF), and the u32 at byte 4 + p equals crc32(row[0 : 4 + p]).  Bytes behind 8 + p are not looked at (the padding of the
 * Hamming and RS modes); a valid row delivers row[4 : 4 + p].  An all-zero row is invalid (crc32 of four zero bytes is 0x2144DF1C),
 * every error burst of at most 32 bits inside row[0 : 8 + p] is caught, any other damage slips through with probability 2^-32.
 * Stage entry points (k_fcs_wrap / k_fcs_check, any context whatever its ecc):
 * wrap: row f = in_dev[f*in_stride .. + len_f), len_f = in_len_dev[f] clamped to [0, n_bytes], or n_bytes when NULL, becomes its
 *   envelope at out_dev[f*out_stride ..]; the bytes behind it, up to n_bytes + 8, are written as 0; out_len_dev[f] (optional) =
 *   len_f + 8.  in_stride >= n_bytes, out_stride >= n_bytes + 8; n_bytes + 8 > INT32_MAX: OFDM_ERR_UNSUPPORTED.
 * check: row f = row_dev[f*row_stride .. + L_f), L_f = row_len_dev[f] clamped to [0, n_row], or n_row when NULL.  Valid: the payload
 *   is written to out_dev[f*out_stride ..], out_len_dev[f] = p, ok_dev[f] = 1.  Invalid: out_len_dev[f] = 0, ok_dev[f] = 0, and the
 *   output row may hold bytes of the rejected payload.  out_len_dev and ok_dev are optional.  row_stride >= n_row, out_stride >=
 *   max(n_row - 8, 0); input and output rows must not overlap.  No byte outside [row, row + L_f) is read whatever the length word says.
 * A violated stride rule, a negative count or a NULL context: OFDM_ERR_INVALID.  n_frames == 0: OFDM_OK, nothing is written.
 *
 * Frame modes ecc = OFDM_ECC_FCS + mode.  Transmit: the frame is mode's frame of E(payload), row by row (a ragged row codes its own
 * len_f); ofdm_coded_len(p), ofdm_data_symbols(p) and ofdm_frame_samples(p) are mode's values at p + 8; payload_bytes + 8 > INT32_MAX:
 * OFDM_ERR_UNSUPPORTED.  Receive: mode's chain runs unchanged; a frame it leaves at OFDM_FRAME_OK with L bytes is checked: valid ->
 * out_len = p, the payload at the start of the output row; invalid -> status OFDM_FRAME_FCS, out_len 0.  A frame with any other status
 * keeps it, with out_len 0.  A frame cut short by the end of the capture fails the check and is reported.  Rows: out_stride >=
 * max(R - 8, 0), R = the row size mode asks for the same max_symbols (OFDM_ERR_INVALID otherwise), in every decode entry point
 * (ofdm_rx_decode_batch, _host, _long, _long_host, a merged detection included). */
int ofdm_fcs_wrap_batch(ofdm_ctx *ctx, const uint8_t *in_dev, int64_t n_frames, int64_t in_stride, const int32_t *in_len_dev,
                        int64_t n_bytes, uint8_t *out_dev, int64_t out_stride, int32_t *out_len_dev);
int ofdm_fcs_check_batch(ofdm_ctx *ctx, const uint8_t *row_dev, int64_t n_frames, int64_t row_stride, const int32_t *row_len_dev,
                         int64_t n_row, uint8_t *out_dev, int64_t out_stride, int32_t *out_len_dev, int32_t *ok_dev);

/* ------------------------------------------------------------------ pipelines */

/* encode (src/transmitter.rs:11-58) for a batch: frame f = [lock][preamble x4][training x5][data symbols],
 * normalised per frame.  payload f = payload_dev[f*payload_stride .. + len_f), len_f = payload_len_dev[f] or
 * payload_bytes when NULL; a len_f outside [0, payload_bytes] is clamped to that range.  EVERY row, the last one included, must be READABLE for payload_bytes bytes whatever its len_f (the
 * kernels prefetch whole rows and mask afterwards): payload_stride >= payload_bytes (OFDM_ERR_INVALID otherwise when n_frames > 1),
 * and the buffer ends no earlier than the last row's payload_bytes.  Every frame is laid out for payload_bytes (D = ofdm_data_symbols(payload_bytes))
 * and written to out_dev[f*out_stride ..] (out_stride >= ofdm_frame_samples(payload_bytes)).
 * With ECC the payload is Hamming(7,4)-encoded first and the header carries the coded length (HAMMING74 and HAMMING74_SOFT alike);
 * with OFDM_ECC_CONV_K7 it is convolutionally encoded (a row of true length len_f codes to 2 (len_f + 1) bytes).  The 16-byte
 * header itself is never coded.  OFDM_ECC_CONV_K7F_*: the framed stream (length block + punctured body) of the row's len_f.
 * OFDM_ECC_LDPC648: the coded info stream of the row's len_f ("LDPC(648,324)" above). */
int ofdm_tx_encode_batch(ofdm_ctx *ctx, const uint8_t *payload_dev, int64_t n_frames, int64_t payload_stride,
                         const int32_t *payload_len_dev, int32_t payload_bytes, ofdm_fc32 *out_dev,
                         int64_t out_stride);

/* decode (src/receiver.rs:9-96) for a batch, with Schmidl-Cox timing/CFO in place of xcorr_fft:
 * sync over n_lags lags -> offset = max(d_hat - L - backoff, 0) -> CFO derotation -> channel estimate ->
 * per symbol FFT / equalise / pilot phase / demap -> 16-byte length header -> truncate [-> Hamming decode].
 * At most max_symbols data symbols per frame are demodulated (fewer if the frame is shorter).
 * out_dev[f*out_stride ..] receives out_len_dev[f] bytes (out_stride >= max_symbols*bytes_per_symbol).
 * status/offset/f_delta/metric are per-frame outputs; any of offset/f_delta/metric may be NULL.
 * ecc = OFDM_ECC_HAMMING74_SOFT (here and in every decode entry point that wraps this one: _host, _long, _long_host): the header is
 * read from hard bits as with HAMMING74, the body from LLR 128 on is ML-decoded from ofdm_rx_llr_batch's LLRs at
 * OFDM_SOFT_LLR_SCALE with the frame's channel estimate; out_len = floor(coded / 7) * 4 as with HAMMING74.
 * ecc = OFDM_ECC_CONV_K7 (likewise in every wrapper): with keep = the header's value if it is below the demodulated body, else the
 * body, the Viterbi decoder runs 4 * keep steps over LLRs 128 .. 128 + 8 keep of the same LLRs, terminated iff the frame was not cut
 * short, and out_len = max(keep / 2 - 1, 0) -- the tail byte is not delivered; out_stride >= max((max_symbols * bytes_per_symbol -
 * 16) / 2 - 1, 0).  A max_symbols whose body exceeds 2^18 bytes (2^20 trellis steps): OFDM_ERR_UNSUPPORTED.
 * ecc = OFDM_ECC_CONV_K7F_* (likewise in every wrapper): the rule of "punctured rates and framed modes" above; status may become
 * OFDM_FRAME_HEADER.  With avail = max(max_symbols * bytes_per_symbol - 16 - 18, 0), out_stride >= floor(T' / 8) for the largest T'
 * with kept(T', rate) <= 8 avail (at most 3 avail / 4); a T' above 2^20: OFDM_ERR_UNSUPPORTED.
 * chest_mode = OFDM_CHEST_WLS (likewise in every wrapper, every ecc): "channel estimate" above is H' of "channel-estimate denoising".
 * cfo_mode = OFDM_CFO_WIDE (likewise in every wrapper, every ecc): "CFO derotation" above uses f_delta + 2 pi m / S of "wide CFO
 * acquisition", and f_delta_dev receives that total offset.
 * ecc = OFDM_ECC_LDPC648 (likewise in every wrapper): the frame rule of "LDPC(648,324)" above; status may become OFDM_FRAME_HEADER or
 * OFDM_FRAME_UNCORRECTABLE; out_stride >= max(40 floor(body_max / 80) - 8, 0).
 * ecc = OFDM_ECC_FCS + mode (likewise in every wrapper): mode's rule above, then the check of "frame check sequence": out_len = the
 * p bytes that were sent, or status OFDM_FRAME_FCS and out_len 0; out_stride >= max(R - 8, 0) with R = mode's row for max_symbols. */
int ofdm_rx_decode_batch(ofdm_ctx *ctx, const ofdm_fc32 *in_dev, int64_t n_frames, int64_t frame_stride,
                         int64_t frame_len, int64_t n_lags, int32_t max_symbols, uint8_t *out_dev,
                         int64_t out_stride, int32_t *out_len_dev, int32_t *status_dev, int32_t *offset_dev,
                         double *f_delta_dev, float *metric_dev);

/* ------------------------------------------------------------------ soft combining (north-star extension)
 * LLR-level (Chase) combining of R = n_branches captures of ONE frame -- two antennas, or a frame received twice.  Parity unpinned by
 * the reference, which has nothing of the kind: tests/combine_ref.py is the definition.  Layout: branch r of frame f is row f * R + r
 * of every per-branch array, so captures [n_frames][R][frame_len] are an ordinary batch of n_frames * R rows.  Per frame:
 *   live       branch r is live iff its status is 0 (or status_dev is NULL), its quality row has OFDM_Q_VALID == 1 and u_r =
 *              OFDM_Q_LLR_UNIT is finite and > 0; without quality rows every branch with status 0 is live and u_r = 1
 *   weights    u_max = the largest u_r over the live branches; q_r = rint(64 (double)u_r / (double)u_max), the IEEE f64 quotient, ties
 *              to even: an integer in [0, OFDM_COMBINE_WEIGHT_ONE].  A dead branch has q_r = 0, and a live one more than about 21 dB
 *              below the best rounds to 0: it is left out (and not read), as intended
 *   counted    branch r counts at positions j < n_r, n_r = n_live_dev[f * R + r] clamped to [0, n_llr], or n_llr without the array (a
 *              branch cut short by the end of its capture)
 *   combined   out[j] = clamp((sum_r q_r L_r[j] + 32) >> 6, -127, 127) over the branches that count at j, the shift arithmetic (floor),
 *              the sum in int32 (at most 8 * 64 * 128 in magnitude); a position at which no branch counts is 0.  With R = 1 this is L
 *              itself, except that -128 becomes -127.  Bytes of the output row behind n_llr are not written.
 * The weights come from link quality because an unweighted sum of a good and a poor capture is worse than the good one alone
 * (profiles/combine_ber_and_speed.json). */
#define OFDM_COMBINE_MAX_BRANCHES 8
#define OFDM_COMBINE_WEIGHT_ONE 64
/* The stage, on any context whatever its ecc: llr_dev rows f * R + r of n_llr int8 LLRs, llr_stride apart -> out_dev rows f, out_stride
 * apart; quality_dev: n_frames * R rows of OFDM_QUALITY_FIELDS floats, or NULL; status_dev, n_live_dev: optional int32 per branch row;
 * weight_dev: optional int32 per branch row, receives q_r.  Rows may start at any address and have any stride >= n_llr (16-byte
 * aligned bases and strides take the 16-byte path).  OFDM_ERR_INVALID: a NULL llr_dev or out_dev with n_frames > 0, a negative size,
 * llr_stride or out_stride < n_llr, n_branches outside 1 .. OFDM_COMBINE_MAX_BRANCHES; n_llr > 2^31 - 2^13: OFDM_ERR_UNSUPPORTED.
 * n_frames == 0: OFDM_OK, nothing is written.  One launch (k_llr_combine), no workspace. */
int ofdm_llr_combine_batch(ofdm_ctx *ctx, const int8_t *llr_dev, int64_t n_frames, int32_t n_branches, int64_t llr_stride, int64_t n_llr,
                           const float *quality_dev, const int32_t *status_dev, const int32_t *n_live_dev, int8_t *out_dev,
                           int64_t out_stride, int32_t *weight_dev);
/* ofdm_rx_decode_batch for frames of R captures each: capture r of frame f = in_dev[(f * R + r) * frame_stride .. + frame_len).
 * Defined as the composition of the stages:
 *   1. per branch row, the front end of ofdm_rx_decode_batch: the context's sync mode, the trimmed start and live symbols, the channel
 *      estimate (chest_mode honoured) -> status_r, offset_r, f_delta_r, nsym_r, H_r
 *   2. the training part of ofdm_rx_quality_batch over the same rows (syms_per_frame = 0, no points, status_r, H_r)
 *   3. ofdm_rx_llr_batch's LLRs at OFDM_SOFT_LLR_SCALE over max_symbols symbols from symbol 10
 *   4. the rule above with n_r = nsym_r * data_carriers * bps; nsym_f = the largest nsym_r over the live branches; status_f = 0 if a
 *      branch is live, otherwise the first non-zero status_r in branch order, or OFDM_FRAME_HEADER if every status_r is 0
 *   5. the mode's finishing step on the combined row with status_f and nsym_f, then its outer layers, as ofdm_rx_decode_batch runs them
 * out_dev / out_stride / out_len_dev / status_dev: per FRAME, out_stride by the mode's rule for ofdm_rx_decode_batch; out_len is 0 for
 * a frame without a live branch.  branch_status_dev, offset_dev, f_delta_dev, metric_dev (the search's), weight_dev (q_r), quality_dev
 * (rows of OFDM_QUALITY_FIELDS): per BRANCH ROW, each optional.  With R = 1 every output equals ofdm_rx_decode_batch's bit for bit.
 * Supported: the modes whose inner code reads nothing from one capture's hard bytes -- OFDM_ECC_CONV_K7F_* and OFDM_ECC_LDPC648 / _R23 /
 * _R34 / _R56, alone or under OFDM_ECC_RS255 and / or OFDM_ECC_FCS; every other mode: OFDM_ERR_UNSUPPORTED.  OFDM_ERR_INVALID as
 * ofdm_rx_decode_batch, and for n_branches outside 1 .. OFDM_COMBINE_MAX_BRANCHES.  The LLR workspace holds R + 1 rows a frame. */
int ofdm_rx_decode_combine_batch(ofdm_ctx *ctx, const ofdm_fc32 *in_dev, int64_t n_frames, int32_t n_branches, int64_t frame_stride,
                                 int64_t frame_len, int64_t n_lags, int32_t max_symbols, uint8_t *out_dev, int64_t out_stride,
                                 int32_t *out_len_dev, int32_t *status_dev, int32_t *branch_status_dev, int32_t *offset_dev,
                                 double *f_delta_dev, float *metric_dev, int32_t *weight_dev, float *quality_dev);

/* ------------------------------------------------------------------ host buffers
 * The reference's encode returns a host Vec<Complex64> and decode consumes one (src/transmitter.rs:11-15, src/receiver.rs:9-13).
 * These entry points take HOST pointers and do the staging inside the library: the batch is cut into chunks of chunk_frames
 * frames (<= 0: about 48 MB of samples) that move through three slots -- H2D of chunk k + 1 on a copy stream, the kernels of chunk k
 * on the context's stream, D2H of chunk k - 1 on a second copy stream.  Page-locked caller memory (ofdm_host_alloc,
 * ofdm_host_register) is DMA-ed in place; pageable memory is staged through pinned bounce buffers by the calling thread (slower:
 * one extra host copy).  The calls are synchronous: results are in the caller's arrays when they return.  Same results, byte for
 * byte, as the device-buffer entry points they wrap. */
int ofdm_host_alloc(size_t bytes, void **host);   /* page-locked host memory (hipHostMalloc) */
int ofdm_host_free(void *host);
int ofdm_host_register(void *host, size_t bytes); /* page-lock memory the caller owns (a Rust Vec's buffer) for the time being */
int ofdm_host_unregister(void *host);
int ofdm_host_is_pinned(const void *host, size_t bytes); /* 1 when [host, host + bytes) can be DMA-ed in place */
/* ofdm_rx_decode_batch on host buffers: frame f = in_host[f*frame_stride .. +frame_len) (frame_stride >= frame_len), outputs as there
 * but in host arrays; offset / f_delta / metric may be NULL. */
int ofdm_rx_decode_host(ofdm_ctx *ctx, const ofdm_fc32 *in_host, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                        int64_t n_lags, int32_t max_symbols, uint8_t *out_host, int64_t out_stride, int32_t *out_len_host,
                        int32_t *status_host, int32_t *offset_host, double *f_delta_host, float *metric_host, int64_t chunk_frames);
/* ofdm_rx_demod_batch on host buffers for regular streams (no offsets, no CFO, H == 1): the BASELINE metric's path. */
int ofdm_rx_demod_host(ofdm_ctx *ctx, const ofdm_fc32 *in_host, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                       int32_t first_symbol, int32_t syms_per_frame, uint8_t *out_host, int64_t out_stride, int64_t chunk_frames);
/* ofdm_tx_encode_batch on host buffers (payload_len_host may be NULL; row f is read for its own length only).  A length above
 * payload_bytes is clamped to payload_bytes, as the device entry point clamps it; the samples are those of ofdm_tx_encode_batch. */
int ofdm_tx_encode_host(ofdm_ctx *ctx, const uint8_t *payload_host, int64_t n_frames, int64_t payload_stride,
                        const int32_t *payload_len_host, int32_t payload_bytes, ofdm_fc32 *out_host, int64_t out_stride,
                        int64_t chunk_frames);

/* ------------------------------------------------------------------ one long capture
 * The reference's receiver hands ONE long buffer to each decode! (examples/jetson_rx.rs:15-17,48-49,84-86: 2 000 000 samples) and
 * looks for the packet anywhere in it (src/receiver.rs:20-25).  A batch of one such frame would occupy one workgroup; here the
 * search runs as a batch of overlapping SLICES of the capture (slice_lags own lags each, <= 0: chosen by the library, plus a
 * read-only halo of 2W + L samples).
 *
 * ofdm_sc_correlate_long: the Schmidl-Cox detection whose first threshold crossing d1 lies in [lag_lo, lag_hi) (lag_hi <= 0: the
 * capture's last lag), with its whole peak window [d1, d1 + W] -- which may reach past lag_hi -- exactly as ONE search over the
 * whole capture evaluates it.  *d_hat = the lag in the capture, -1 if none; f_delta / metric optional.  A host that splits the
 * lags of one capture over several contexts / GPUs (ofdm_amd.dist.halo_ranges) takes the answer of the lowest range that has one.
 * Synchronous; d_hat, f_delta, metric are HOST pointers. */
int ofdm_sc_correlate_long(ofdm_ctx *ctx, const ofdm_fc32 *in_dev, int64_t n_samples, int64_t lag_lo, int64_t lag_hi,
                           int64_t slice_lags, int64_t *d_hat, double *f_delta, float *metric);
/* decode (src/receiver.rs:9-96) of ONE long capture: the search above over [lag_lo, lag_hi) (skipped when d_hat_known >= 0: a
 * detection merged from several contexts), then the receive chain from that frame on.  With the whole lag range it is identical to
 * ofdm_rx_decode_batch with n_frames = 1 on the whole capture: status, offset (into the capture), CFO, metric, bytes -- except that
 * a capture without a detection (OFDM_FRAME_NOSYNC) reports f_delta = metric = 0 without running the chain.  With lag_lo > 0 the
 * detection is the first crossing at or after lag_lo (lags in front of it are never looked at, although the frame's own first
 * samples may lie there), i.e. the result of ofdm_rx_decode_batch on the capture from lag_lo on, re-based to the whole capture.  out_dev[0 .. out_cap) is a DEVICE
 * buffer (out_cap as out_stride there); out_len, status, offset, f_delta, metric are HOST pointers (the last three optional).
 * With sync_mode = OFDM_SYNC_REFERENCE the lag range must be the whole capture. */
int ofdm_rx_decode_long(ofdm_ctx *ctx, const ofdm_fc32 *in_dev, int64_t n_samples, int64_t lag_lo, int64_t lag_hi,
                        int64_t d_hat_known, int32_t max_symbols, uint8_t *out_dev, int64_t out_cap, int32_t *out_len,
                        int32_t *status, int64_t *offset, double *f_delta, float *metric);
/* the same from and to host memory: what `decode!(samples)` of a 2 M-sample Vec is */
int ofdm_rx_decode_long_host(ofdm_ctx *ctx, const ofdm_fc32 *in_host, int64_t n_samples, int32_t max_symbols, uint8_t *out_host,
                             int64_t out_cap, int32_t *out_len, int32_t *status, int64_t *offset, double *f_delta, float *metric);

/* ------------------------------------------------------------------ every packet of one long capture (EXT-12)
 * A capture holds many packets; the calls above find the first one of a lag range.  ofdm_sc_scan_long finds every detection of
 * [lag_lo, lag_hi) in one pass (k_sc_mark + k_sc_walk + k_sc_peaks: three launches and one synchronisation whatever the count).
 * OFDM_SYNC_SCHMIDL_COX only; any other sync mode: OFDM_ERR_UNSUPPORTED.
 *
 * The rule, in the notation of the oracle's orc_sc_sync (L = S, W = sync_window_reps L, num = |P|^2, den = E R, thr the context's
 * threshold, valid = n_samples - W - L + 1, lag_hi <= 0 or > valid: valid):
 *     lo_0 = lag_lo
 *     detection k:  d1_k = the first lag d in [lo_k, lag_hi) with den(d) > 0 and num(d) >= thr den(d)      (none: the scan ends)
 *                   d_hat_k = the first maximum of M = num / den over [d1_k, min(d1_k + W, valid - 1)], compared as orc_sc_sync
 *                             compares (num bden > bnum den); the window may reach past lag_hi
 *                   f_delta_k = atan2(P(d_hat_k)) / L,  metric_k = num / den at d_hat_k
 *     lo_{k+1} = d1_k + holdoff                                                                              (holdoff >= 1)
 *     the scan ends after max_det detections; *more = 1 iff a further detection exists
 * For every k this is orc_sc_sync(capture[lo_k:]) re-based by lo_k, and, whenever lag_hi > d1_k, the answer of
 * ofdm_sc_correlate_long(lag_lo = lo_k, lag_hi).  Every lag's sums are the oracle's own, bit for bit (the W products of that window,
 * in order), so d1 and d_hat are the oracle's at any margin; they depend on the capture and the rule only, never on the grid.
 *
 * holdoff is the caller's knowledge of the traffic: with fixed-size frames ofdm_frame_samples(payload) - W or a little less; without
 * that knowledge a small value, and the decode's status sorts out a false detection inside a payload (the framed, LDPC and frame-check
 * modes report it as OFDM_FRAME_HEADER / OFDM_FRAME_FCS).  holdoff = 1 on a plateau yields one detection per crossing lag.
 *
 * in_dev is a DEVICE pointer; d1, d_hat (int64), f_delta, metric (max_det entries each; d1, f_delta, metric optional), n_det and more
 * (optional) are HOST pointers; entries at or beyond *n_det are not written.  Synchronous.  The next search would start at
 * d1[n_det - 1] + holdoff: with *more set, call again with that lag_lo.  Decode packet k with ofdm_rx_decode_long(lag_lo = lo_k, lag_hi).
 * OFDM_ERR_INVALID: holdoff < 1, max_det < 0, n_samples < 0, lag_lo < 0, a NULL in_dev with n_samples > 0, a NULL d_hat or n_det.
 * OFDM_ERR_UNSUPPORTED: n_samples > 2^40.  A capture with no valid lag: *n_det = 0 and OFDM_OK. */
int ofdm_sc_scan_long(ofdm_ctx *ctx, const ofdm_fc32 *in_dev, int64_t n_samples, int64_t lag_lo, int64_t lag_hi, int64_t holdoff,
                      int64_t max_det, int64_t *d1, int64_t *d_hat, double *f_delta, float *metric, int64_t *n_det, int32_t *more);
/* the same on a capture in host memory (uploaded as ofdm_rx_decode_long_host uploads its capture; pinned memory is DMA-ed in place) */
int ofdm_sc_scan_long_host(ofdm_ctx *ctx, const ofdm_fc32 *in_host, int64_t n_samples, int64_t lag_lo, int64_t lag_hi, int64_t holdoff,
                           int64_t max_det, int64_t *d1, int64_t *d_hat, double *f_delta, float *metric, int64_t *n_det, int32_t *more);

/* ------------------------------------------------------------------ every packet of one long capture in one batched decode (EXT-13)
 * ofdm_rx_decode_packets decodes the packets k = 0 .. n_det - 1 of a capture of n samples in ONE run of the receive chain, given the
 * triples (d_hat_k, f_delta_k, M_k) exactly as ofdm_sc_scan_long returns them.  Nothing here refers to the slice search of
 * ofdm_rx_decode_long: the timing IS the scan's values (in-order sums, the oracle's bit for bit, independent of grid and lag_lo).
 *
 * The rule (L = S, b = sync_backoff; numpy restatement: tests/packets_ref.py).  Packet k is steps 2 - 5 of ofdm_rx_decode_batch on the
 * sub-capture capture[r_k:] with known timing:
 *     row start      r_k = max(d_hat_k - L - b, 0) & ~1; the row-relative peak is d_hat_k - r_k, the row's own length n - r_k
 *     timing fields  off = max(d_hat - L - b, 0) (row-relative); OFDM_FRAME_SHORT below 10 L samples behind it;
 *                    ns = min(ceil(len / L) - 10, max_symbols) live symbols; status -4 if ns bytes_per_symbol < 16
 *     CFO            f_delta_k through the context's cfo_mode as the chain puts it through: OFDM_CFO_OFF -> 0, OFDM_CFO_ABS -> |.|,
 *                    OFDM_CFO_WIDE -> plus 2 pi m / S from k_cfo_wide; chest_mode, the LLR weight and every ecc apply unchanged
 *     outputs        bytes, out_len, status: the chain's; offset (int64, into the capture) = r_k + the row's offset (0 + the row's
 *                    where the chain reports OFDM_FRAME_BADTIMING, as ofdm_rx_decode_long); f_delta = the value the chain derotated
 *                    with; metric = M_k, passed through bit for bit
 * On the device the rows are an ordinary batch: k_gather_rows copies capture[r_k : r_k + R] into row k of a workspace,
 * R = min((10 + max_symbols) S + 2, n rounded up to even), zeros at and beyond sample n, and k_rx_prepare_rows gives a row cut by the
 * capture's end the live symbols of its true length.  The packets are walked in chunks whose rows stay within 256 MiB.  A row depends
 * on its own triple and the capture only: not on the other packets, their order, the chunking or the grid.
 *
 * in_dev (8-byte aligned) and the outputs are DEVICE pointers (offset_dev, f_delta_dev, metric_dev optional); d_hat, f_delta, metric
 * are HOST arrays of n_det entries, read before the call returns unless they are page-locked (then: unchanged until the stream
 * reaches the end of the call).  Asynchronous on the context's stream, like ofdm_rx_decode_batch; out_stride: its rule.
 * OFDM_ERR_INVALID: a d_hat entry outside [0, n_samples) (checked on the host before any launch), n_det < 0, n_samples < 0,
 * max_symbols <= 0, a NULL required pointer, an out_stride below the row size.  OFDM_ERR_UNSUPPORTED: a sync mode other than
 * OFDM_SYNC_SCHMIDL_COX, n_samples > 2^40, n_det >= 2^31.  n_det = 0: OFDM_OK with no launch. */
int ofdm_rx_decode_packets(ofdm_ctx *ctx, const ofdm_fc32 *in_dev, int64_t n_samples, int64_t n_det, const int64_t *d_hat,
                           const double *f_delta, const float *metric, int32_t max_symbols, uint8_t *out_dev, int64_t out_stride,
                           int32_t *out_len_dev, int32_t *status_dev, int64_t *offset_dev, double *f_delta_dev, float *metric_dev);
/* A capture in host memory (uploaded as ofdm_rx_decode_long_host uploads its capture): ofdm_sc_scan_long(lag_lo, lag_hi, holdoff,
 * max_det), then ofdm_rx_decode_packets with the scan's rows, into HOST arrays: out_host = max_det rows of out_stride bytes, out_len,
 * status, offset (optional), f_delta, metric per packet, and d1 (optional), d_hat, *n_det, *more (optional) as the scan reports them.
 * Two synchronisations whatever the packet count.  Errors: those of the two calls. */
int ofdm_rx_decode_all_long_host(ofdm_ctx *ctx, const ofdm_fc32 *in_host, int64_t n_samples, int64_t lag_lo, int64_t lag_hi,
                                 int64_t holdoff, int64_t max_det, int32_t max_symbols, uint8_t *out_host, int64_t out_stride,
                                 int32_t *out_len, int32_t *status, int64_t *offset, double *f_delta, float *metric, int64_t *d1,
                                 int64_t *d_hat, int64_t *n_det, int32_t *more);

/* ------------------------------------------------------------------ sc16 receive input (EXT-9)
 * Radios deliver sc16 -- interleaved little-endian int16 I and Q, 4 bytes a sample: UHD's wire format and that of most recorded
 * captures -- not fc32.  The sample format is a property of a CALL, not of a context: the same context decodes fc32 and sc16.
 *
 * Widen:   x = (float)v * scale for each component v.  The conversion is exact; the product is ONE f32 multiplication, rounded to
 *          nearest even, and it is rounded before anything else uses it: it is never contracted into a following add or FMA.  (HIP
 *          compiles with -ffp-contract=fast, under which __fmul_rn is a plain `*`; the kernels issue the product as its own
 *          v_mul_f32 instruction from inline assembly, which is equivalent to a non-contracted __fmul_rn.)  numpy's
 *          i16.astype(np.float32) * np.float32(scale) is the same number for every input and every scale, so every sc16 entry
 *          point returns bit for bit what its fc32 twin returns on the widened samples.
 * Narrow:  (the transmit side, for a DAC)  y = x * scale, the same single rounded product; q = rint(y), ties to even, clamped to
 *          [-32767, 32767] (-32768 is never produced); a NaN gives 0.  A component COUNTS AS CLIPPED when y is not finite or rint(y)
 *          lies outside [-32767, 32767]; the count is one int32 a frame.
 * scale must be finite and > 0, otherwise OFDM_ERR_INVALID. */
typedef struct { int16_t re, im; } ofdm_sc16;   /* interleaved, little-endian: UHD's sc16 */
#define OFDM_SC16_DEFAULT_SCALE (1.0f / 32768.0f)
/* The definition in C, on the host (no device, no context): n samples.  clipped (optional): clipped components of the whole call. */
int ofdm_sc16_widen(const ofdm_sc16 *in, int64_t n, float scale, ofdm_fc32 *out);
int ofdm_sc16_narrow(const ofdm_fc32 *in, int64_t n, float scale, ofdm_sc16 *out, int64_t *clipped);
/* The same on the device (k_sc16_widen / k_sc16_narrow): n_frames rows of frame_len samples, strides in samples, stride >= frame_len
 * on both sides; rows may start at any sample (4-byte alignment on the sc16 side, 8 on the fc32 side; 16-byte accesses are used when
 * bases and strides allow them).  Nothing behind frame_len in an output row is written.  clipped_dev (optional): int32 per frame.
 * Negative sizes, or NULL buffers with work to do: OFDM_ERR_INVALID; n_frames == 0: OFDM_OK and nothing is written. */
int ofdm_sc16_widen_batch(ofdm_ctx *ctx, const ofdm_sc16 *in_dev, int64_t n_frames, int64_t in_stride, int64_t frame_len, float scale,
                          ofdm_fc32 *out_dev, int64_t out_stride);
int ofdm_sc16_narrow_batch(ofdm_ctx *ctx, const ofdm_fc32 *in_dev, int64_t n_frames, int64_t in_stride, int64_t frame_len, float scale,
                           ofdm_sc16 *out_dev, int64_t out_stride, int32_t *clipped_dev);
/* ofdm_rx_demod_batch on sc16 samples (in_dev 4-byte aligned).  N = 64 inside the fast path's envelope -- no offset / f_delta / soft
 * output, H shared or absent, a multiple of 8 symbols wholly inside frame_len, out_dev and out_stride multiples of 4 -- runs
 * k_demod64_sc16, which reads the int16 pairs itself (half the bytes of k_demod64).  Everything else is widened by k_sc16_widen, a chunk
 * of frames (about 48 MB of widened samples) at a time, into a workspace and goes through ofdm_rx_demod_batch's own dispatch. */
int ofdm_rx_demod_sc16_batch(ofdm_ctx *ctx, const ofdm_sc16 *in_dev, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                             float scale, int32_t first_symbol, int32_t syms_per_frame, const int32_t *offset_dev,
                             const double *f_delta_dev, const ofdm_fc32 *hk_dev, int64_t hk_stride, uint8_t *out_dev,
                             int64_t out_stride, ofdm_fc32 *soft_dev);
/* ofdm_rx_decode_batch on sc16 captures: k_sc16_widen per chunk of frames into the same workspace, then the unchanged chain on the chunk
 * (every ecc, chest_mode, cfo_mode and sync_mode of the context); per-frame outputs land at the chunk's offset. */
int ofdm_rx_decode_sc16_batch(ofdm_ctx *ctx, const ofdm_sc16 *in_dev, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                              float scale, int64_t n_lags, int32_t max_symbols, uint8_t *out_dev, int64_t out_stride,
                              int32_t *out_len_dev, int32_t *status_dev, int32_t *offset_dev, double *f_delta_dev, float *metric_dev);
/* The two host-buffer calls (see "host buffers") on sc16 host arrays: half the H2D bytes of their fc32 twins, the same outputs. */
int ofdm_rx_demod_sc16_host(ofdm_ctx *ctx, const ofdm_sc16 *in_host, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                            float scale, int32_t first_symbol, int32_t syms_per_frame, uint8_t *out_host, int64_t out_stride,
                            int64_t chunk_frames);
int ofdm_rx_decode_sc16_host(ofdm_ctx *ctx, const ofdm_sc16 *in_host, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                             float scale, int64_t n_lags, int32_t max_symbols, uint8_t *out_host, int64_t out_stride,
                             int32_t *out_len_host, int32_t *status_host, int32_t *offset_host, double *f_delta_host,
                             float *metric_host, int64_t chunk_frames);

/* ------------------------------------------------------------------ sc16 transmit output and sc16 long captures (EXT-10)
 * ofdm_tx_encode_batch writing sc16 for a DAC: row f of out_dev is, bit for bit, ofdm_sc16_narrow(frame f of ofdm_tx_encode_batch on the
 * same arguments, scale) -- every component is formed exactly as the fc32 entry point forms it and then narrowed by the rule above --
 * and clipped_dev[f] (optional, int32 per frame) is that function's count for the frame.  Samples of an output row behind
 * ofdm_frame_samples(payload_bytes) are not written.  Every ecc, every N, ragged payload_len.
 * A NORMALISED FRAME IS NOT BOUNDED BY +-1.  normalize (src/transmitter.rs:183-194) divides by the SIGNED maximum of the frame's
 * components: the positive peak is 1, the negative peak is whatever it is -- about -2 for BPSK and QPSK without guard bands (the
 * reference's default shape), where EVERY frame has a component that clips at scale 32767; about -1.2 for 16-QAM with guard bands; inside
 * +-1 for 64-QAM and 256-QAM with guard bands.  clipped_dev is how a caller learns that its scale is too large for the frames it sends;
 * the library does not choose a scale.
 * Argument rules: those of ofdm_tx_encode_batch, and scale finite and > 0 (OFDM_ERR_INVALID); out_dev needs 4-byte alignment only.
 * N = 64 frames of 1 .. 56 data symbols into a 16-byte aligned out_dev with out_stride a multiple of 4 samples run k_txframe64_sc16,
 * which narrows in its store phase (4 bytes a sample written, nothing else).  Everything else -- longer frames, N != 64, an unaligned
 * output -- runs ofdm_tx_encode_batch's own kernels on a chunk of frames (about 48 MB of fc32 samples) into a workspace and then
 * k_sc16_narrow into the caller's rows. */
int ofdm_tx_encode_sc16_batch(ofdm_ctx *ctx, const uint8_t *payload_dev, int64_t n_frames, int64_t payload_stride,
                              const int32_t *payload_len_dev, int32_t payload_bytes, float scale,
                              ofdm_sc16 *out_dev, int64_t out_stride, int32_t *clipped_dev /* optional, per frame */);
/* The same on host buffers (see "host buffers"; ofdm_tx_encode_host's rules): half the D2H bytes of the fc32 call.  clipped_host
 * (optional): int32 per frame, brought back with each chunk's frames. */
int ofdm_tx_encode_sc16_host(ofdm_ctx *ctx, const uint8_t *payload_host, int64_t n_frames, int64_t payload_stride,
                             const int32_t *payload_len_host, int32_t payload_bytes, float scale,
                             ofdm_sc16 *out_host, int64_t out_stride, int32_t *clipped_host /* optional */, int64_t chunk_frames);
/* ofdm_rx_decode_long / ofdm_rx_decode_long_host (see "one long capture") on an sc16 capture: every output -- status, length, offset,
 * the bits of f_delta and metric, the bytes -- equals the fc32 call on ofdm_sc16_widen(capture, scale), for every ecc, chest_mode,
 * cfo_mode, sync_mode, lag range and d_hat_known.  in_dev is 4-byte aligned.  The capture is widened on the device by k_sc16_widen into
 * a buffer the context keeps (8 bytes a sample), and the chain runs on that: the host call uploads 4 bytes a sample instead of 8, and
 * the device then holds 12 bytes a sample (the int16 capture and its widened copy) where the fc32 call holds 8. */
int ofdm_rx_decode_long_sc16(ofdm_ctx *ctx, const ofdm_sc16 *in_dev, int64_t n_samples, float scale, int64_t lag_lo, int64_t lag_hi,
                             int64_t d_hat_known, int32_t max_symbols, uint8_t *out_dev, int64_t out_cap, int32_t *out_len,
                             int32_t *status, int64_t *offset, double *f_delta, float *metric);
int ofdm_rx_decode_long_sc16_host(ofdm_ctx *ctx, const ofdm_sc16 *in_host, int64_t n_samples, float scale, int32_t max_symbols,
                                  uint8_t *out_host, int64_t out_cap, int32_t *out_len, int32_t *status, int64_t *offset,
                                  double *f_delta, float *metric);

/* ------------------------------------------------------------------ a streaming receiver (EXT-14)
 * A radio hands over a few thousand samples at a time, without end, and packets straddle the buffers.  A stream takes the samples as they
 * come (ofdm_stream_push) and delivers every packet exactly once: HOWEVER THE STREAM IS CUT INTO PUSHES, THE PACKETS DELIVERED ARE, FIELD
 * FOR FIELD AND BIT FOR BIT, THOSE OF ONE ofdm_rx_decode_all_long_host CALL ON THE CONCATENATION.  (The declarations stand behind the sc16
 * sections because the sc16 push needs ofdm_sc16; the rules are EXT-12's and EXT-13's.)
 *
 * Notation: sample 0 is the first sample pushed after create or reset, T the number pushed so far; S, L = S, W, b = sync_backoff and
 * valid = T - W - L + 1 as in the EXT-12 text; max_symbols and holdoff mean what they mean in ofdm_rx_decode_all_long_host; max_chunk is
 * the largest number of samples the stream's buffers take at once (a larger push is walked in pieces inside the call).
 *     reference   A(T) = ofdm_rx_decode_all_long_host(stream[0:T], lag_lo = 0, lag_hi = 0, holdoff, max_det unbounded, max_symbols):
 *                 detections k = 0, 1, .. with d1_k, d_hat_k and per packet status, out_len, bytes, offset, f_delta, metric
 *     horizon     H = W + (10 + max_symbols) S + 2; detection k is COMMITTED at T iff d1_k + H <= T.  Then its peak window [d1_k, d1_k + W]
 *                 lies below valid (sync_window_reps <= 3) and its whole gathered row [r_k, r_k + R) inside the stream (0 <= b <= cp_len),
 *                 so every field of packet k in A(T) is its field in A(T') for all T' >= T (the proof in integers: tests/test_stream_cpu.py)
 *     push        without flush: delivers, in order, every committed detection not delivered before; a detection that is not committed
 *                 defers itself and every later one.  So packet k arrives in the result of the first push after which T >= d1_k + H, or in
 *                 the flush, and in no other: the delivery time is part of the contract
 *     flush       delivers every remaining detection of A(T), a last frame cut by the end of the stream with the prefix the one-shot call
 *                 delivers.  Then the stream is ended: a further push is OFDM_ERR_INVALID until ofdm_stream_reset
 *     first_sample (create and reset, any int64 >= 0) is added to the reported d1, d_hat and offset and to nothing else: every rule
 *                 above, the `& ~1` of the row start included, is in stream-relative indices.  It exists for timestamps
 * The sums of every lag's window are the oracle's own in order and the timing triple is the scan's (EXT-12, EXT-13), "a row depends on
 * its own triple and the capture only": that is what makes the answer exact and not merely close.
 *
 * Per piece of a push the stream runs k_stream_ingest<fc32> / k_stream_ingest<sc16> (ONE launch: the samples it keeps from the old window
 * and the new chunk into the other window), ofdm_sc_scan_long's kernels over the window from the lag the walk resumes at, and
 * ofdm_rx_decode_packets' chain over the committed detections: ofdm_last_dispatch names them in that order (a push that delivers nothing:
 * the ingest and the scan; a window that has no valid lag yet: the ingest alone; a flush with n = 0: no ingest), once -- the pieces behind
 * the first of a push larger than max_chunk are left out.  The window keeps the samples from (lo - L - b) & ~1 on, lo = the first lag
 * not yet decided (a deferred detection's d1, else max(the last d1 + holdoff, valid)): never more than H + L + b + 2 + max_chunk samples,
 * sized once at create.  The stream owns its windows, its staging buffer and its result rows (freed by ofdm_stream_destroy) and uses the
 * context's workspaces call by call: several streams on one context are independent.  Pushes are synchronous on the context's stream; a
 * stream is no more thread-safe than its context, and is destroyed BEFORE its context.
 *
 * in_host: n samples in host memory (pinned memory is DMA-ed in place).  The outputs are HOST arrays of max_pkt entries, laid out as in
 * ofdm_rx_decode_all_long_host (out_host: rows of out_stride bytes; offset, d1 and more optional).  *n_pkt = the packets delivered by this
 * call; *more = 1: deliverable packets remain beyond max_pkt -- call again with n = 0 and the same flush to drain them; a flush is
 * complete when it returns more = 0.  n = 0 without flush and with nothing pending is a no-op with *n_pkt = 0.
 * ofdm_stream_push_sc16 is ofdm_stream_push on ofdm_sc16_widen(in, scale), bit for bit, widened on the device; scale is per push and
 * follows the rule of the other sc16 entry points.
 * ofdm_stream_state (all outputs optional): T, the first sample the window keeps, lo, and whether the stream is ended (stream-relative).
 * OFDM_ERR_INVALID: a NULL handle, n < 0, NULL in_host with n > 0, holdoff < 1, max_symbols <= 0, max_chunk <= 0, first_sample < 0,
 * max_pkt < 0, a NULL required output, an out_stride below the decode row size, a bad sc16 scale, a push on an ended stream.
 * OFDM_ERR_UNSUPPORTED: a context whose sync_mode is not OFDM_SYNC_SCHMIDL_COX or a max_chunk beyond 2^40 (at create), T beyond 2^40.
 * A push that fails leaves the stream undefined until ofdm_stream_reset. */
typedef struct ofdm_stream ofdm_stream;
int ofdm_stream_create(ofdm_stream **out, ofdm_ctx *ctx, int32_t max_symbols, int64_t holdoff, int64_t max_chunk, int64_t first_sample);
int ofdm_stream_destroy(ofdm_stream *s);
int ofdm_stream_reset(ofdm_stream *s, int64_t first_sample);
int ofdm_stream_push(ofdm_stream *s, const ofdm_fc32 *in_host, int64_t n, int32_t flush, int64_t max_pkt, uint8_t *out_host,
                     int64_t out_stride, int32_t *out_len, int32_t *status, int64_t *offset, double *f_delta, float *metric, int64_t *d1,
                     int64_t *d_hat, int64_t *n_pkt, int32_t *more);
int ofdm_stream_push_sc16(ofdm_stream *s, const ofdm_sc16 *in_host, int64_t n, float scale, int32_t flush, int64_t max_pkt,
                          uint8_t *out_host, int64_t out_stride, int32_t *out_len, int32_t *status, int64_t *offset, double *f_delta,
                          float *metric, int64_t *d1, int64_t *d_hat, int64_t *n_pkt, int32_t *more);
int ofdm_stream_state(const ofdm_stream *s, int64_t *total, int64_t *kept_from, int64_t *next_lag, int32_t *ended);

/* ------------------------------------------------------------------ a DC blocker in front of detection (EXT-15)
 * A direct-conversion radio adds a constant (LO leakage) to every sample.  The Schmidl-Cox metric of a constant is 1 at every lag: a DC
 * term 3.8 dB above the noise floor fires the detector on noise alone and no packet behind it is ever timed.  With guard bands the DC
 * bin carries nothing, so the constant can be taken out in front of the detector.  Opt-in everywhere; off, nothing changes.
 *
 * Definition (numpy: tests/dcblock_ref.py; parity with the reference is unpinned: it has nothing of the kind).  x[0 .. n) is fc32 -- an
 * sc16 stream first widened as ofdm_sc16_widen does, x = (float)v * scale, one rounded product.  blocks = M, 1 <= M <= 1024.  Real and
 * imaginary parts are treated alike and independently.
 *     block sums  Samples form blocks of 64, aligned at sample 0 of the filter's stream (a reset starts a new stream at 0).  A complete
 *                 block j has the sum b_j, formed in f64 by the balanced pairwise tree: s = the block's 64 samples as f64, then six
 *                 times s = s[0::2] + s[1::2].  A block that is not complete has no sum and is never history.
 *     output      sample i lies in block j = i / 64; lo = max(j - M, 0).  lo == j (block 0): y[i] = x[i].  Otherwise acc = b_lo, then
 *                 acc += b_k for k = lo + 1 .. j - 1 in ascending order, in f64; m = acc / (64 (j - lo)) in f64; m32 = (float)m, rounded
 *                 to nearest even; y[i] = x[i] - m32 in f32.
 * The mean never contains the sample's own block: the filter has no latency, a stream's sample count and delivery rule stay what they
 * are.  Nothing is special-cased for non-finite samples: a NaN spoils the M blocks behind its own block, per IEEE (which NaN: unspecified).
 * Known and accepted: the first 64 samples of a stream pass unfiltered (L >= 80: no Schmidl-Cox product has both factors in them); without
 * guard bands the DC bin carries data, and the filter disturbs it.
 * ofdm_dc_block_default = ceil(3 S / 64), S = n_fft + cp_len (4 blocks at n_fft = 64, 60 at 1024): the middle of the band that works --
 * a window of S or less follows the real-valued locking block and loses the frame, one of 8 S still holds the locking block during the
 * training blocks.  OFDM_ERR_INVALID (< 0) for sizes ofdm_create refuses.
 *
 * ofdm_dc_block / ofdm_dc_block_sc16: the definition on host arrays, one whole stream, no GPU (out may not alias in).
 * OFDM_ERR_INVALID: n < 0, blocks outside 1 .. 1024, a NULL array with n > 0, a bad sc16 scale; OFDM_ERR_UNSUPPORTED: n beyond 2^40;
 * OFDM_ERR_NOMEM: the n / 64 block sums cannot be allocated.
 * The handle (ofdm_dcblock_*) is the filter on DEVICE buffers, enqueued on the context's stream: the pushes of a handle, concatenated,
 * equal ofdm_dc_block of the concatenated inputs bit for bit, however the stream is cut.  One launch per piece (k_dc_block<fc32> /
 * k_dc_block<sc16>; a push longer than max_chunk is walked in pieces, ofdm_last_dispatch names the first); the handle owns its state
 * (the last M block sums and the open block's samples, double-buffered) and is destroyed BEFORE its context.  n = 0 is a no-op.
 * OFDM_ERR_INVALID: a NULL handle or context, blocks outside 1 .. 1024, max_chunk <= 0, n < 0, a NULL buffer with n > 0, a bad sc16
 * scale, in_dev and out_dev overlapping.  OFDM_ERR_UNSUPPORTED: max_chunk or n beyond 2^40.
 *
 * ofdm_stream_set_dc_block: the filter in front of a stream's window (0 = off, the default; blocks outside 0 .. 1024 or a NULL handle:
 * OFDM_ERR_INVALID).  Only while the stream's total is 0, else OFDM_ERR_INVALID; ofdm_stream_reset keeps the setting and clears the
 * history.  The first setting that is not 0 allocates the filter's state and a second staging buffer of max_chunk samples
 * (OFDM_ERR_NOMEM), kept until ofdm_stream_destroy.  ofdm_stream_get_dc_block: the setting.  With it on, a push is bit for bit the push of the
 * filtered samples, and the contract of EXT-14 carries over word for word: the packets are those of ONE ofdm_rx_decode_all_long_host on
 * ofdm_dc_block(concatenation, blocks) -- ofdm_dc_block_sc16(concatenation, scale, blocks) for sc16 pushes -- each delivered exactly
 * once, with the push EXT-14's rule names; T and H are unchanged.  Per piece k_dc_block<fc32> / <sc16> runs between the upload and
 * k_stream_ingest<fc32> (also for sc16 pushes: the filtered chunk is fc32) and leads the dispatch string. */
int ofdm_dc_block_default(int32_t n_fft, int32_t cp_len);
int ofdm_dc_block(const ofdm_fc32 *in, int64_t n, int32_t blocks, ofdm_fc32 *out);
int ofdm_dc_block_sc16(const ofdm_sc16 *in, int64_t n, float scale, int32_t blocks, ofdm_fc32 *out);
typedef struct ofdm_dcblock ofdm_dcblock;
int ofdm_dcblock_create(ofdm_dcblock **out, ofdm_ctx *ctx, int32_t blocks, int64_t max_chunk);
int ofdm_dcblock_destroy(ofdm_dcblock *f);
int ofdm_dcblock_reset(ofdm_dcblock *f);
int ofdm_dcblock_push(ofdm_dcblock *f, const ofdm_fc32 *in_dev, int64_t n, ofdm_fc32 *out_dev);
int ofdm_dcblock_push_sc16(ofdm_dcblock *f, const ofdm_sc16 *in_dev, int64_t n, float scale, ofdm_fc32 *out_dev);
int ofdm_dcblock_state(const ofdm_dcblock *f, int64_t *total, int32_t *blocks);
int ofdm_stream_set_dc_block(ofdm_stream *s, int32_t blocks);
int ofdm_stream_get_dc_block(const ofdm_stream *s, int32_t *blocks);

/* ------------------------------------------------------------------ a digital down-converter: tune, filter, decimate (EXT-16)
 * A radio delivers a few fixed rates, is usually tuned off-centre (LO leakage, 1/f noise), and the band it hands over often holds a
 * neighbour.  The down-converter shifts the wanted signal to 0, low-passes and keeps every D-th sample, so that everything behind it
 * runs at the modem's own rate.  Opt-in everywhere; off, nothing changes.
 *
 * Definition (numpy: tests/ddc_ref.py; parity with the reference is unpinned: it has nothing of the kind).  IEEE basic operations only,
 * so host, device and numpy agree bit for bit:
 *     inputs      x[0 .. n) fc32 -- an sc16 stream first widened as ofdm_sc16_widen does, one rounded product; decim = D, 1 .. 64;
 *                 h[0 .. T) real f32 taps, D <= T <= 4096; phase_inc, any int32, taken mod 2^20.
 *     rotors      C[i] = (f32 cos(2 pi i / 1024), f32 sin(2 pi i / 1024)), F[i] = (f32 cos(2 pi i / 2^20), f32 sin(2 pi i / 2^20)), i < 1024:
 *                 formed once in f64 on the host and rounded to f32; ofdm_ddc_rotor_tables hands out the very bytes the host definition
 *                 uses and the device is given (coarse, fine: 2048 floats each, re and im interleaved).
 *     a (x) b     re = fmaf(a.re, b.re, -(a.im * b.im)), im = fmaf(a.re, b.im, a.im * b.re); the inner product is ONE rounded f32
 *                 multiply, nothing else is contracted.
 *     mixer       sample n (the absolute index since create / reset, int64) has the phase p = (n * phase_inc) mod 2^20 in exact integer
 *                 arithmetic; r = C[p >> 10] (x) F[p & 1023]; v[n] = x[n] (x) r.
 *     filter      y[m] = sum_{k = 0}^{T - 1} h[k] v[m D + k] for 0 <= m < M(n); M(n) = 0 for n < T, else (n - T) / D + 1.  Each part
 *                 starts from +0.0 and runs in ascending k as acc = fmaf(h[k], v.part, acc).  No zero padding, no latency bookkeeping:
 *                 an output exists when its T inputs exist.
 * Nothing is special-cased for non-finite samples: a NaN at sample n spoils exactly the outputs whose window holds n.
 *
 * ofdm_ddc / ofdm_ddc_sc16: the definition on host arrays, one whole stream, no GPU.  out receives M(n) samples (*n_out; out_cap < M(n):
 * OFDM_ERR_INVALID, nothing written).  ofdm_ddc_out_len: M(n), or OFDM_ERR_INVALID (< 0) for arguments the others refuse.
 * ofdm_ddc_inc_for: the increment that brings f0 (cycles per input sample) to 0, (-rint(f0 2^20)) mod 2^20; OFDM_ERR_INVALID for a
 * non-finite f0 or |f0| > 0.5.  ofdm_ddc_design: a Hamming-windowed sinc of T = taps_per_phase D taps (taps_per_phase 1 .. 64) with the
 * cutoff 0.5 / D, formed in f64, normalised to sum 1, rounded to f32: h[k] = w(k) sinc((k - (T - 1) / 2) / D), w(k) = 0.54 - 0.46
 * cos(2 pi k / (T - 1)) (T = 1: h = [1]).  The taps are an input of everything else, as the pilot tables are: a caller may bring its own.
 * OFDM_ERR_INVALID: n < 0, decim outside 1 .. 64, n_taps outside decim .. 4096, a NULL array that is needed, a bad sc16 scale;
 * OFDM_ERR_UNSUPPORTED: n beyond 2^40.
 *
 * The handle (ofdm_ddc_create .. ofdm_ddc_state) is the converter on DEVICE buffers, enqueued on the context's stream: the outputs of
 * a handle's pushes, concatenated, equal ofdm_ddc of the concatenated inputs bit for bit, however the stream is cut.  A push of n
 * samples writes M(total + n) - M(total) outputs (*n_out; out_cap below that: OFDM_ERR_INVALID, nothing is launched).  One launch per
 * piece (k_ddc<fc32> / k_ddc<sc16>; a push longer than max_chunk is walked in pieces, ofdm_last_dispatch names the first).  The handle
 * owns its state -- the taps, the rotor tables and the last <= T - 1 raw samples, the latter double-buffered and written by the same
 * launch -- and allocates nothing after create; destroy it BEFORE its context.  in_dev is on 8 bytes (sc16: 4), out_dev on 8, and they do
 * not overlap.  ofdm_ddc_state: the samples taken and the samples given since create / reset.
 * OFDM_ERR_INVALID: a NULL handle or context, the argument ranges above, max_chunk <= 0, n < 0, a NULL or misaligned buffer with n > 0,
 * in_dev and out_dev overlapping; OFDM_ERR_UNSUPPORTED: max_chunk or n beyond 2^40.
 *
 * ofdm_stream_set_ddc: the converter in front of a stream (decim = 0: off, the default, and then bit for bit the stream without it;
 * taps NULL with n_taps = 0: ofdm_ddc_design with OFDM_DDC_TAPS_PER_PHASE).  Only while the stream's total is 0, else OFDM_ERR_INVALID;
 * ofdm_stream_reset keeps the setting and clears the history.  The first setting that is not 0 allocates the converter's state and a
 * staging buffer (OFDM_ERR_NOMEM), kept until ofdm_stream_destroy.  Pushes are then INPUT-rate samples (at most max_chunk a piece);
 * per piece k_ddc<fc32> / <sc16> runs between the upload and everything the stream did before, and leads the dispatch string; the DC
 * blocker, if set, runs on the converter's output.  T, H, holdoff, first_sample, the totals of ofdm_stream_state and every offset are in
 * OUTPUT samples, and the contract of EXT-14 carries over word for word on the converted samples: the packets are those of ONE
 * ofdm_rx_decode_all_long_host on ofdm_ddc(concatenation) -- ofdm_ddc_sc16 for sc16 pushes, ofdm_dc_block of that if the DC blocker is
 * set -- each delivered exactly once; packet k arrives with the first push after which the output count reaches d1_k + H, or with the
 * flush.  ofdm_stream_get_ddc: decim, phase_inc (mod 2^20) and n_taps of the setting (any may be NULL).
 * Not covered: several channels from one read of the input (a polyphase channeliser), rational resampling, complex taps, a phase
 * offset, chunks already on the device, the converter on batches of rows, OFDM_SYNC_REFERENCE. */
#define OFDM_DDC_TAPS_PER_PHASE 24
#define OFDM_DDC_MAX_DECIM 64
#define OFDM_DDC_MAX_TAPS 4096
int ofdm_ddc_rotor_tables(float *coarse, float *fine);
int64_t ofdm_ddc_out_len(int64_t n, int32_t decim, int32_t n_taps);
int ofdm_ddc_inc_for(double f0_cycles_per_sample, int32_t *inc);
int ofdm_ddc_design(int32_t decim, int32_t taps_per_phase, float *taps);
int ofdm_ddc(const ofdm_fc32 *in, int64_t n, int32_t decim, int32_t phase_inc, const float *taps, int32_t n_taps, ofdm_fc32 *out,
             int64_t out_cap, int64_t *n_out);
int ofdm_ddc_sc16(const ofdm_sc16 *in, int64_t n, float scale, int32_t decim, int32_t phase_inc, const float *taps, int32_t n_taps,
                  ofdm_fc32 *out, int64_t out_cap, int64_t *n_out);
typedef struct ofdm_ddc_handle ofdm_ddc_handle;
int ofdm_ddc_create(ofdm_ddc_handle **out, ofdm_ctx *ctx, int32_t decim, int32_t phase_inc, const float *taps, int32_t n_taps,
                    int64_t max_chunk);
int ofdm_ddc_destroy(ofdm_ddc_handle *h);
int ofdm_ddc_reset(ofdm_ddc_handle *h);
int ofdm_ddc_push(ofdm_ddc_handle *h, const ofdm_fc32 *in_dev, int64_t n, ofdm_fc32 *out_dev, int64_t out_cap, int64_t *n_out);
int ofdm_ddc_push_sc16(ofdm_ddc_handle *h, const ofdm_sc16 *in_dev, int64_t n, float scale, ofdm_fc32 *out_dev, int64_t out_cap,
                       int64_t *n_out);
int ofdm_ddc_state(const ofdm_ddc_handle *h, int64_t *total_in, int64_t *total_out);
int ofdm_stream_set_ddc(ofdm_stream *s, int32_t decim, int32_t phase_inc, const float *taps, int32_t n_taps);
int ofdm_stream_get_ddc(const ofdm_stream *s, int32_t *decim, int32_t *phase_inc, int32_t *n_taps);

/* ------------------------------------------------------------------ loop-back test bench
 * channel (src/channel.rs:33-74), per frame:
 *     y = convolve(tx, CHANNEL)                          tx_len + 63 samples (CHANNEL: the 64 taps of channel.rs:26-31)
 *     timing_error:  y[i] *= exp(+j f (i + 1)),  f = pi U(0,1) / 80                                   (channel.rs:48-62)
 *     y[i] += sqrt(0.5 var / snr) (U(-1,1) + j U(-1,1)),  var = the complex pseudo-variance of y, snr = 10^(snr_db/10)
 * The reference draws from an unseeded thread_rng; here frame f draws from SplitMix64(seed + f) in the reference's order
 * (f first when timing_error, then re, im per sample) -- the stream oracle/ofdm_oracle.c:orc_channel uses, so the two can be
 * compared sample by sample.  Test-bench extensions, NULL = the reference's behaviour: delay_dev[f] >= 0 places the channel
 * output at out + delay[f] (what does not fit out_len is dropped; every one of the out_len slot samples receives noise, the
 * samples outside the channel output nothing else), f_delta_in_dev[f] replaces the drawn CFO (any sign).
 * out_len >= tx_len + 63, out_stride >= out_len.  f_delta_out_dev (optional): the CFO applied to each frame. */
int ofdm_channel_batch(ofdm_ctx *ctx, const ofdm_fc32 *tx_dev, int64_t n_frames, int64_t tx_stride, int64_t tx_len,
                       double snr_db, int32_t timing_error, uint64_t seed, const int32_t *delay_dev,
                       const double *f_delta_in_dev, ofdm_fc32 *out_dev, int64_t out_stride, int64_t out_len,
                       double *f_delta_out_dev);
int ofdm_channel_taps(double *taps64); /* CHANNEL (src/channel.rs:26-31). Host call. */

/* ------------------------------------------------------------------ measurement helpers
 * HIP events on the context's stream, so a host without HIP bindings can time kernels (bench.py). */
/* Read-only stream over n_symbols 80-sample (640-byte) symbols at in_dev, nothing but the loads: the practical HBM read
 * ceiling of an access pattern, to read the demod kernel's rate against.  pattern 0 = the N = 64 demod kernel's access
 * (8-byte loads, the 128-byte cyclic prefix of every symbol never touched), 1 = the same loads over whole symbols,
 * 2 = unit-stride 16-byte loads.  Enqueued on the context's stream; time it with ofdm_timer_start / _stop_ms. */
int ofdm_hbm_read_probe(ofdm_ctx *ctx, const ofdm_fc32 *in_dev, int64_t n_symbols, int32_t pattern);
int ofdm_timer_start(ofdm_ctx *ctx);
int ofdm_timer_stop_ms(ofdm_ctx *ctx, float *elapsed_ms); /* records, synchronises, returns elapsed */

#ifdef __cplusplus
}
#endif
#endif /* OFDM_HIP_H */
