//! bindings/ofdm_hip.rs -- Rust FFI for libofdm_hip.so (include/ofdm_hip.h).
//!
//! UNTESTED SOURCE TEXT: the authoring image has no cargo/rustc.  It shows the binding a
//! maintainer of jkelleyrtp/ofdm would add as `src/ofdm_hip.rs` so that `encode` / `decode`
//! (src/transmitter.rs:11-58, src/receiver.rs:9-96) keep their signatures while the DSP runs on an MI355X.
#![allow(non_camel_case_types, dead_code)]
use num::complex::Complex64;
use std::os::raw::{c_char, c_int, c_void};

#[repr(C)]
pub struct ofdm_ctx { _private: [u8; 0] }
#[repr(C)]
pub struct ofdm_stream { _private: [u8; 0] }
#[repr(C)]
pub struct ofdm_dcblock { _private: [u8; 0] }
#[repr(C)]
pub struct ofdm_ddc_handle { _private: [u8; 0] }

#[repr(C)]
#[derive(Clone, Copy)]
pub struct ofdm_fc32 { pub re: f32, pub im: f32 }

// EXT-9: interleaved little-endian int16 I/Q (UHD's sc16); x = v as f32 * scale, one rounded f32 product (include/ofdm_hip.h)
#[repr(C)]
#[derive(Clone, Copy)]
pub struct ofdm_sc16 { pub re: i16, pub im: i16 }
pub const OFDM_SC16_DEFAULT_SCALE: f32 = 1.0 / 32768.0;

#[repr(C)]
#[derive(Clone, Copy)]
pub struct ofdm_params {
    pub n_fft: i32, pub cp_len: i32, pub modulation: i32, pub guard_bands: i32, pub ecc: i32,
    pub sync_window_reps: i32, pub sync_backoff: i32, pub cfo_mode: i32, pub sync_threshold: f32,
    pub sync_mode: i32,
    pub rx_path: i32,
    pub chest_mode: i32,
    pub reserved: [i32; 4],
}

pub const OFDM_OK: c_int = 0;
pub const OFDM_FRAME_SHORT: i32 = -1; // "Input not long enough, bailing early" (src/receiver.rs:27-29)
pub const OFDM_MOD_BPSK: i32 = 1;
pub const OFDM_MOD_QPSK: i32 = 2;
pub const OFDM_MOD_QAM16: i32 = 4;
pub const OFDM_MOD_QAM64: i32 = 6;
pub const OFDM_ECC_NONE: i32 = 0;
pub const OFDM_ECC_HAMMING74: i32 = 1;
// same frames on the wire as OFDM_ECC_HAMMING74; decode ML-decodes the code from int8 LLRs (include/ofdm_hip.h)
pub const OFDM_ECC_HAMMING74_SOFT: i32 = 2;
// K = 7 rate-1/2 convolutional code (133 / 171 octal), zero-terminated by one tail byte, Viterbi-decoded from int8 LLRs; 3 and 4 are
// not modes (include/ofdm_hip.h)
pub const OFDM_ECC_CONV_K7: i32 = 5;
// framed convolutional modes: a rate-1/2 coded length block that decode reads instead of the uncoded header, then the payload at rate
// 1/2, 2/3 or 3/4 (punctured); parity unpinned by the reference, tests/framed_ref.py is the definition (include/ofdm_hip.h)
pub const OFDM_ECC_CONV_K7F_R12: i32 = 10;
pub const OFDM_ECC_CONV_K7F_R23: i32 = 11;
pub const OFDM_ECC_CONV_K7F_R34: i32 = 12;
// outer Reed-Solomon(255,223) around the frames of an inner mode, 20 + inner (inner = OFDM_ECC_NONE or a framed mode): the reference's
// create_transmission_bytes / decipher_transmission_bytes inside encode / decode, on the device (include/ofdm_hip.h)
pub const OFDM_ECC_RS255: i32 = 20;
pub const OFDM_ECC_RS255_K7F_R12: i32 = 30;
pub const OFDM_ECC_RS255_K7F_R23: i32 = 31;
pub const OFDM_ECC_RS255_K7F_R34: i32 = 32;
pub const OFDM_FRAME_UNCORRECTABLE: i32 = -5; // OFDM_ECC_RS255*: an RS block with more than 16 byte errors (the reference returns None); OFDM_ECC_LDPC648: an unconverged code word
// LDPC(648,324), rate 1/2, layered normalised min-sum from LLRs; the length travels in the first code word; parity unpinned by the
// reference, tests/ldpc_ref.py is the definition (include/ofdm_hip.h)
pub const OFDM_ECC_LDPC648: i32 = 16;
// the project's own LDPC(648) codes of rates 2/3, 3/4 and 5/6 under the same frame rule (K = 53 / 60 / 67 info bytes a code word);
// `rate` of the ofdm_ldpc648_*_rate functions: 0 = 1/2, 1 = 2/3, 2 = 3/4, 3 = 5/6
pub const OFDM_ECC_LDPC648_R23: i32 = 41;
pub const OFDM_ECC_LDPC648_R34: i32 = 42;
pub const OFDM_ECC_LDPC648_R56: i32 = 43;
pub const OFDM_LDPC_MAX_ITER: i32 = 20;
// CRC-32 frame check around any of the fifteen modes above, 64 + mode: decode delivers exactly the payload that was sent or reports
// the frame with OFDM_FRAME_FCS; parity unpinned by the reference, tests/fcs_ref.py is the definition (include/ofdm_hip.h)
pub const OFDM_ECC_FCS: i32 = 64;
pub const OFDM_FCS_OVERHEAD: i64 = 8;
pub const OFDM_FRAME_FCS: i32 = -6;
pub const OFDM_CONV_RATE_1_2: i32 = 0;
pub const OFDM_CONV_RATE_2_3: i32 = 1;
pub const OFDM_CONV_RATE_3_4: i32 = 2;
pub const OFDM_SOFT_LLR_SCALE: f32 = 32.0;
// ofdm_params.chest_mode: the reference's bin-by-bin estimate (default), or that estimate denoised by a weighted least-squares fit of
// cp_len taps -- opt-in, receive side only; parity unpinned by the reference, tests/chest_ref.py is the definition (include/ofdm_hip.h)
pub const OFDM_CHEST_LS: i32 = 0;
pub const OFDM_CHEST_WLS: i32 = 1;
// ofdm_params.cfo_mode.  OFF, SIGNED (default) and ABS work with the Schmidl-Cox phase alone, which is defined modulo 2 pi / S
// rad/sample: an acquisition range of +-pi / S, +-0.4 sub-carrier spacings.  WIDE resolves the whole multiples of 2 pi / S from the
// training blocks (ofdm_cfo_wide_batch with span = OFDM_CFO_WIDE_SPAN behind the Schmidl-Cox search of every decode entry point):
// +-6.8 sub-carrier spacings.  OFDM_SYNC_SCHMIDL_COX only; opt-in, receive side only; parity unpinned by the reference,
// tests/cfo_wide_ref.py is the definition (include/ofdm_hip.h)
pub const OFDM_CFO_OFF: i32 = 0;
pub const OFDM_CFO_SIGNED: i32 = 1;
pub const OFDM_CFO_ABS: i32 = 2;
pub const OFDM_CFO_WIDE: i32 = 3;
pub const OFDM_CFO_WIDE_SPAN: i32 = 8;
pub const OFDM_CFO_WIDE_MAX_SPAN: i32 = 32;
// ofdm_set_llr_weight (EXT-11): what the decode chains weigh their LLRs by -- the channel weight alone (default), or that times the
// per-carrier noise weight q_k measured from the training blocks
pub const OFDM_LLRW_CHANNEL: i32 = 0;
pub const OFDM_LLRW_NOISE: i32 = 1;
// ofdm_rx_quality_batch: indices into a frame's row of OFDM_QUALITY_FIELDS floats (noise variance, gain, linear SNR, LLR unit, linear
// EVM^2, counted points); parity unpinned by the reference, tests/quality_ref.py is the definition (include/ofdm_hip.h)
pub const OFDM_Q_VALID: usize = 0;
pub const OFDM_Q_NOISE_VAR: usize = 1;
pub const OFDM_Q_GAIN: usize = 2;
pub const OFDM_Q_SNR: usize = 3;
pub const OFDM_Q_LLR_UNIT: usize = 4;
pub const OFDM_Q_EVM2: usize = 5;
pub const OFDM_Q_POINTS: usize = 6;
pub const OFDM_QUALITY_FIELDS: usize = 8;
// ofdm_llr_combine_batch / ofdm_rx_decode_combine_batch (EXT-7 soft combining): at most this many captures of one frame, and the weight
// of the best live one; parity unpinned by the reference, tests/combine_ref.py is the definition (include/ofdm_hip.h)
pub const OFDM_COMBINE_MAX_BRANCHES: i32 = 8;
pub const OFDM_COMBINE_WEIGHT_ONE: i32 = 64;

/// The crate's own `ModulationScheme` (src/transmitter.rs:98-104) is what `encode` / `decode` keep taking.  Its `Qam` arm is
/// empty in the reference (transmitter.rs:135-136, receiver.rs:185: "Only 16 qam is implemented"); here it selects 16-QAM.
use crate::ModulationScheme;
fn bits_per_point(m: &ModulationScheme) -> i32 {
    match m {
        ModulationScheme::Bpsk => OFDM_MOD_BPSK,
        ModulationScheme::Qpsk => OFDM_MOD_QPSK,
        ModulationScheme::Qam => OFDM_MOD_QAM16,
    }
}

#[link(name = "ofdm_hip")]
extern "C" {
    pub fn ofdm_abi_version() -> c_int;
    pub fn ofdm_strerror(status: c_int) -> *const c_char;
    pub fn ofdm_device_count(count: *mut c_int) -> c_int;
    pub fn ofdm_default_params(p: *mut ofdm_params) -> c_int;
    pub fn ofdm_default_pilots(n_fft: i32, cp_len: i32, preamble: *mut f64, training: *mut f64) -> c_int;
    pub fn ofdm_stdrng_pilots(n_fft: i32, cp_len: i32, preamble: *mut f64, training: *mut f64) -> c_int;
    pub fn ofdm_rs255_encoded_len(n_bytes: i64) -> i64;
    pub fn ofdm_rs255_decoded_len(n_code: i64) -> i64;
    pub fn ofdm_rs255_encode(data: *const u8, n_bytes: i64, out: *mut u8) -> c_int;
    pub fn ofdm_rs255_decode(code: *const u8, n_code: i64, out: *mut u8, corrected: *mut i32) -> c_int;
    pub fn ofdm_tx_symbols_batch(ctx: *mut ofdm_ctx, bytes_dev: *const u8, n_bytes: i64, out_dev: *mut ofdm_fc32, n_sym: i64) -> c_int;
    pub fn ofdm_crc32(data: *const u8, n_bytes: i64) -> u32;
    pub fn ofdm_chacha_block(key8: *const u32, words12_15: *const u32, rounds: i32, out16: *mut u32) -> c_int;
    pub fn ofdm_create(p: *const ofdm_params, preamble: *const f64, training: *const f64, device: c_int,
                       stream: *mut c_void, out: *mut *mut ofdm_ctx) -> c_int;
    pub fn ofdm_destroy(ctx: *mut ofdm_ctx) -> c_int;
    pub fn ofdm_set_stream(ctx: *mut ofdm_ctx, stream: *mut c_void) -> c_int;
    pub fn ofdm_synchronize(ctx: *mut ofdm_ctx) -> c_int;
    pub fn ofdm_last_hip_error(ctx: *const ofdm_ctx) -> c_int;
    pub fn ofdm_last_dispatch(ctx: *const ofdm_ctx, buf: *mut c_char, n: usize) -> c_int;
    pub fn ofdm_set_tuning(ctx: *mut ofdm_ctx, key: *const c_char, value: i64) -> c_int;
    pub fn ofdm_get_tuning(ctx: *const ofdm_ctx, key: *const c_char, value: *mut i64) -> c_int;
    pub fn ofdm_dev_alloc(ctx: *mut ofdm_ctx, bytes: usize, dev: *mut *mut c_void) -> c_int;
    pub fn ofdm_dev_free(ctx: *mut ofdm_ctx, dev: *mut c_void) -> c_int;
    pub fn ofdm_memcpy_h2d(ctx: *mut ofdm_ctx, dev: *mut c_void, host: *const c_void, bytes: usize) -> c_int;
    pub fn ofdm_memcpy_d2h(ctx: *mut ofdm_ctx, host: *mut c_void, dev: *const c_void, bytes: usize) -> c_int;
    pub fn ofdm_memset(ctx: *mut ofdm_ctx, dev: *mut c_void, value: c_int, bytes: usize) -> c_int;
    pub fn ofdm_symbol_len(ctx: *const ofdm_ctx) -> c_int;
    pub fn ofdm_data_carriers(ctx: *const ofdm_ctx) -> c_int;
    pub fn ofdm_bytes_per_symbol(ctx: *const ofdm_ctx) -> c_int;
    pub fn ofdm_coded_len(ctx: *const ofdm_ctx, payload_bytes: i64) -> i64;
    pub fn ofdm_data_symbols(ctx: *const ofdm_ctx, payload_bytes: i64) -> i64;
    pub fn ofdm_frame_samples(ctx: *const ofdm_ctx, payload_bytes: i64) -> i64;
    pub fn ofdm_fft_batch(ctx: *mut ofdm_ctx, in_dev: *const ofdm_fc32, out_dev: *mut ofdm_fc32, n_vec: i64, inverse: c_int) -> c_int;
    pub fn ofdm_ifft_cp_batch(ctx: *mut ofdm_ctx, freq_dev: *const ofdm_fc32, out_dev: *mut ofdm_fc32, n_sym: i64) -> c_int;
    pub fn ofdm_unprefix_batch(ctx: *mut ofdm_ctx, in_dev: *const ofdm_fc32, out_dev: *mut ofdm_fc32, n_sym: i64) -> c_int;
    pub fn ofdm_qam_map_batch(ctx: *mut ofdm_ctx, bytes_dev: *const u8, n_bytes: i64, out_dev: *mut ofdm_fc32) -> c_int;
    pub fn ofdm_qam_demap_batch(ctx: *mut ofdm_ctx, sym_dev: *const ofdm_fc32, n_sym: i64, bytes_dev: *mut u8, idx_dev: *mut u8) -> c_int;
    pub fn ofdm_encode_block_batch(ctx: *mut ofdm_ctx, data_dev: *const ofdm_fc32, bins_dev: *mut ofdm_fc32, n_sym: i64) -> c_int;
    pub fn ofdm_normalize_batch(ctx: *mut ofdm_ctx, x_dev: *mut ofdm_fc32, n_frames: i64, frame_stride: i64, frame_len: i64) -> c_int;
    pub fn ofdm_hamming74_encode(ctx: *mut ofdm_ctx, in_dev: *const u8, n_bytes: i64, out_dev: *mut u8) -> c_int;
    pub fn ofdm_hamming74_decode(ctx: *mut ofdm_ctx, in_dev: *const u8, n_bytes: i64, out_dev: *mut u8, corrected_dev: *mut u32) -> c_int;
    pub fn ofdm_hamming74_decode_soft(ctx: *mut ofdm_ctx, llr_dev: *const i8, n_bits: i64, out_dev: *mut u8) -> c_int;
    pub fn ofdm_conv_k7_encode(ctx: *mut ofdm_ctx, in_dev: *const u8, n_frames: i64, in_stride: i64, n_bytes: i64, out_dev: *mut u8,
                               out_stride: i64) -> c_int;
    pub fn ofdm_conv_k7_decode_soft(ctx: *mut ofdm_ctx, llr_dev: *const i8, n_frames: i64, llr_stride: i64, n_steps: i64,
                                    terminated: i32, out_dev: *mut u8, out_stride: i64) -> c_int;
    pub fn ofdm_conv_k7_kept_bits(n_steps: i64, rate: i32) -> i64;
    pub fn ofdm_conv_k7_encode_punctured(ctx: *mut ofdm_ctx, in_dev: *const u8, n_frames: i64, in_stride: i64, n_bytes: i64, rate: i32,
                                         out_dev: *mut u8, out_stride: i64) -> c_int;
    pub fn ofdm_conv_k7_decode_punctured(ctx: *mut ofdm_ctx, llr_dev: *const i8, n_frames: i64, llr_stride: i64, n_steps: i64, rate: i32,
                                         terminated: i32, out_dev: *mut u8, out_stride: i64) -> c_int;
    pub fn ofdm_rs255_encode_batch(ctx: *mut ofdm_ctx, in_dev: *const u8, n_frames: i64, in_stride: i64, in_len_dev: *const i32, n_bytes: i64,
                                   out_dev: *mut u8, out_stride: i64) -> c_int;
    pub fn ofdm_rs255_decode_batch(ctx: *mut ofdm_ctx, code_dev: *const u8, n_frames: i64, code_stride: i64, code_len_dev: *const i32,
                                   n_code: i64, out_dev: *mut u8, out_stride: i64, out_len_dev: *mut i32, corrected_dev: *mut i32) -> c_int;
    pub fn ofdm_ldpc648_coded_len(payload_bytes: i64) -> i64;
    pub fn ofdm_ldpc648_encode(info: *const u8, n_cw: i64, code: *mut u8) -> c_int;
    pub fn ofdm_ldpc648_decode(llr: *const i8, n_cw: i64, max_iter: i32, out: *mut u8, iters: *mut i32) -> c_int;
    pub fn ofdm_ldpc648_encode_batch(ctx: *mut ofdm_ctx, in_dev: *const u8, n_frames: i64, in_stride: i64, n_cw: i64, out_dev: *mut u8,
                                     out_stride: i64) -> c_int;
    pub fn ofdm_ldpc648_decode_batch(ctx: *mut ofdm_ctx, llr_dev: *const i8, n_frames: i64, llr_stride: i64, n_cw: i64, max_iter: i32,
                                     out_dev: *mut u8, out_stride: i64, iters_dev: *mut i32) -> c_int;
    pub fn ofdm_ldpc648_info_bytes(rate: i32) -> i32;
    pub fn ofdm_ldpc648_coded_len_rate(payload_bytes: i64, rate: i32) -> i64;
    pub fn ofdm_ldpc648_encode_rate(info: *const u8, n_cw: i64, rate: i32, code: *mut u8) -> c_int;
    pub fn ofdm_ldpc648_decode_rate(llr: *const i8, n_cw: i64, max_iter: i32, rate: i32, out: *mut u8, iters: *mut i32) -> c_int;
    pub fn ofdm_ldpc648_encode_rate_batch(ctx: *mut ofdm_ctx, in_dev: *const u8, n_frames: i64, in_stride: i64, n_cw: i64, rate: i32,
                                          out_dev: *mut u8, out_stride: i64) -> c_int;
    pub fn ofdm_ldpc648_decode_rate_batch(ctx: *mut ofdm_ctx, llr_dev: *const i8, n_frames: i64, llr_stride: i64, n_cw: i64, max_iter: i32,
                                          rate: i32, out_dev: *mut u8, out_stride: i64, iters_dev: *mut i32) -> c_int;
    pub fn ofdm_fcs_wrap_batch(ctx: *mut ofdm_ctx, in_dev: *const u8, n_frames: i64, in_stride: i64, in_len_dev: *const i32, n_bytes: i64,
                               out_dev: *mut u8, out_stride: i64, out_len_dev: *mut i32) -> c_int;
    pub fn ofdm_fcs_check_batch(ctx: *mut ofdm_ctx, row_dev: *const u8, n_frames: i64, row_stride: i64, row_len_dev: *const i32,
                                n_row: i64, out_dev: *mut u8, out_stride: i64, out_len_dev: *mut i32, ok_dev: *mut i32) -> c_int;
    pub fn ofdm_sc_correlate_batch(ctx: *mut ofdm_ctx, in_dev: *const ofdm_fc32, n_frames: i64, frame_stride: i64, frame_len: i64,
                                   n_lags: i64, d_hat_dev: *mut i32, f_delta_dev: *mut f64, metric_dev: *mut f32) -> c_int;
    pub fn ofdm_frequency_correction_batch(ctx: *mut ofdm_ctx, in_dev: *const ofdm_fc32, n_pairs: i64, stride: i64,
                                           right_offset: i64, f_delta_dev: *mut f64) -> c_int;
    pub fn ofdm_cfo_rotate_batch(ctx: *mut ofdm_ctx, x_dev: *mut ofdm_fc32, n_frames: i64, frame_stride: i64, frame_len: i64,
                                 f_delta_dev: *const f64, first_index_dev: *const i32) -> c_int;
    pub fn ofdm_estimate_channel_batch(ctx: *mut ofdm_ctx, in_dev: *const ofdm_fc32, n_frames: i64, frame_stride: i64,
                                       frame_len: i64, offset_dev: *const i32, f_delta_dev: *const f64, hk_dev: *mut ofdm_fc32) -> c_int;
    pub fn ofdm_chest_matrix(n_fft: i32, cp_len: i32, training: *const f64, rinv: *mut f64) -> c_int;
    pub fn ofdm_chest_smooth_batch(ctx: *mut ofdm_ctx, hk_in_dev: *const ofdm_fc32, n_frames: i64, hk_out_dev: *mut ofdm_fc32) -> c_int;
    pub fn ofdm_chest_window(ctx: *const ofdm_ctx, first_tap: *mut i32, n_taps: *mut i32) -> c_int;
    pub fn ofdm_rx_demod_batch(ctx: *mut ofdm_ctx, in_dev: *const ofdm_fc32, n_frames: i64, frame_stride: i64, frame_len: i64,
                               first_symbol: i32, syms_per_frame: i32, offset_dev: *const i32, f_delta_dev: *const f64,
                               hk_dev: *const ofdm_fc32, hk_stride: i64, out_dev: *mut u8, out_stride: i64, soft_dev: *mut ofdm_fc32) -> c_int;
    pub fn ofdm_rx_llr_batch(ctx: *mut ofdm_ctx, in_dev: *const ofdm_fc32, n_frames: i64, frame_stride: i64, frame_len: i64,
                             first_symbol: i32, syms_per_frame: i32, offset_dev: *const i32, f_delta_dev: *const f64,
                             hk_dev: *const ofdm_fc32, hk_stride: i64, llr_scale: f32, llr_dev: *mut i8, llr_stride: i64) -> c_int;
    pub fn ofdm_rx_quality_batch(ctx: *mut ofdm_ctx, in_dev: *const ofdm_fc32, n_frames: i64, frame_stride: i64, frame_len: i64,
                                 first_symbol: i32, syms_per_frame: i32, n_points_dev: *const i32, offset_dev: *const i32,
                                 f_delta_dev: *const f64, hk_dev: *const ofdm_fc32, hk_stride: i64, status_dev: *const i32,
                                 quality_dev: *mut f32) -> c_int;
    // in/out f_delta_dev: f0 -> f0 + 2 pi m / S; status_dev, m_dev and metric_dev (2 floats per frame) may be null; 1 <= span <= 32
    pub fn ofdm_cfo_wide_batch(ctx: *mut ofdm_ctx, in_dev: *const ofdm_fc32, n_frames: i64, frame_stride: i64, frame_len: i64,
                               offset_dev: *const i32, status_dev: *const i32, span: i32, f_delta_dev: *mut f64, m_dev: *mut i32,
                               metric_dev: *mut f32) -> c_int;
    // EXT-11 noise-aware LLR weights (tests/noise_weight_ref.py is the definition): per-bin noise variance s_k and weight q_k from the
    // scatter of the five training blocks; ofdm_rx_llr_batch with per-bin weights; the per-context mode of the decode chains
    pub fn ofdm_rx_noise_bins_batch(ctx: *mut ofdm_ctx, in_dev: *const ofdm_fc32, n_frames: i64, frame_stride: i64, frame_len: i64,
                                    offset_dev: *const i32, f_delta_dev: *const f64, status_dev: *const i32, nvar_dev: *mut f32,
                                    weight_dev: *mut f32) -> c_int;
    pub fn ofdm_rx_llr_weighted_batch(ctx: *mut ofdm_ctx, in_dev: *const ofdm_fc32, n_frames: i64, frame_stride: i64, frame_len: i64,
                                      first_symbol: i32, syms_per_frame: i32, offset_dev: *const i32, f_delta_dev: *const f64,
                                      hk_dev: *const ofdm_fc32, hk_stride: i64, llr_scale: f32, llr_dev: *mut i8, llr_stride: i64,
                                      bin_weight_dev: *const f32, bin_weight_stride: i64) -> c_int;
    pub fn ofdm_set_llr_weight(ctx: *mut ofdm_ctx, mode: i32) -> c_int;
    pub fn ofdm_get_llr_weight(ctx: *const ofdm_ctx, mode: *mut i32) -> c_int;
    pub fn ofdm_llr_combine_batch(ctx: *mut ofdm_ctx, llr_dev: *const i8, n_frames: i64, n_branches: i32, llr_stride: i64, n_llr: i64,
                                  quality_dev: *const f32, status_dev: *const i32, n_live_dev: *const i32, out_dev: *mut i8,
                                  out_stride: i64, weight_dev: *mut i32) -> c_int;
    pub fn ofdm_rx_decode_combine_batch(ctx: *mut ofdm_ctx, in_dev: *const ofdm_fc32, n_frames: i64, n_branches: i32, frame_stride: i64,
                                        frame_len: i64, n_lags: i64, max_symbols: i32, out_dev: *mut u8, out_stride: i64,
                                        out_len_dev: *mut i32, status_dev: *mut i32, branch_status_dev: *mut i32, offset_dev: *mut i32,
                                        f_delta_dev: *mut f64, metric_dev: *mut f32, weight_dev: *mut i32, quality_dev: *mut f32) -> c_int;
    pub fn ofdm_tx_encode_batch(ctx: *mut ofdm_ctx, payload_dev: *const u8, n_frames: i64, payload_stride: i64,
                                payload_len_dev: *const i32, payload_bytes: i32, out_dev: *mut ofdm_fc32, out_stride: i64) -> c_int;
    pub fn ofdm_rx_decode_batch(ctx: *mut ofdm_ctx, in_dev: *const ofdm_fc32, n_frames: i64, frame_stride: i64, frame_len: i64,
                                n_lags: i64, max_symbols: i32, out_dev: *mut u8, out_stride: i64, out_len_dev: *mut i32,
                                status_dev: *mut i32, offset_dev: *mut i32, f_delta_dev: *mut f64, metric_dev: *mut f32) -> c_int;
    pub fn ofdm_xcorr_batch(ctx: *mut ofdm_ctx, a_dev: *const ofdm_fc32, n_frames: i64, a_stride: i64, a_len: i64, b_dev: *const ofdm_fc32, nb: i32, idx_max_dev: *mut i32, peak_dev: *mut f32, out_dev: *mut ofdm_fc32, out_stride: i64) -> c_int;
    pub fn ofdm_channel_batch(ctx: *mut ofdm_ctx, tx_dev: *const ofdm_fc32, n_frames: i64, tx_stride: i64, tx_len: i64, snr_db: f64, timing_error: i32, seed: u64, delay_dev: *const i32, f_delta_in_dev: *const f64, out_dev: *mut ofdm_fc32, out_stride: i64, out_len: i64, f_delta_out_dev: *mut f64) -> c_int;
    pub fn ofdm_channel_taps(taps64: *mut f64) -> c_int;
    pub fn ofdm_hbm_read_probe(ctx: *mut ofdm_ctx, in_dev: *const ofdm_fc32, n_symbols: i64, pattern: i32) -> c_int;
    pub fn ofdm_use_own_stream(ctx: *mut ofdm_ctx) -> c_int;
    pub fn ofdm_host_alloc(bytes: usize, host: *mut *mut c_void) -> c_int;
    pub fn ofdm_host_free(host: *mut c_void) -> c_int;
    pub fn ofdm_host_register(host: *mut c_void, bytes: usize) -> c_int;
    pub fn ofdm_host_unregister(host: *mut c_void) -> c_int;
    pub fn ofdm_host_is_pinned(host: *const c_void, bytes: usize) -> c_int;
    pub fn ofdm_rx_decode_host(ctx: *mut ofdm_ctx, in_host: *const ofdm_fc32, n_frames: i64, frame_stride: i64, frame_len: i64, n_lags: i64,
                               max_symbols: i32, out_host: *mut u8, out_stride: i64, out_len_host: *mut i32, status_host: *mut i32,
                               offset_host: *mut i32, f_delta_host: *mut f64, metric_host: *mut f32, chunk_frames: i64) -> c_int;
    pub fn ofdm_rx_demod_host(ctx: *mut ofdm_ctx, in_host: *const ofdm_fc32, n_frames: i64, frame_stride: i64, frame_len: i64,
                              first_symbol: i32, syms_per_frame: i32, out_host: *mut u8, out_stride: i64, chunk_frames: i64) -> c_int;
    pub fn ofdm_tx_encode_host(ctx: *mut ofdm_ctx, payload_host: *const u8, n_frames: i64, payload_stride: i64, payload_len_host: *const i32,
                               payload_bytes: i32, out_host: *mut ofdm_fc32, out_stride: i64, chunk_frames: i64) -> c_int;
    pub fn ofdm_sc_correlate_long(ctx: *mut ofdm_ctx, in_dev: *const ofdm_fc32, n_samples: i64, lag_lo: i64, lag_hi: i64, slice_lags: i64,
                                  d_hat: *mut i64, f_delta: *mut f64, metric: *mut f32) -> c_int;
    pub fn ofdm_rx_decode_long(ctx: *mut ofdm_ctx, in_dev: *const ofdm_fc32, n_samples: i64, lag_lo: i64, lag_hi: i64, d_hat_known: i64,
                               max_symbols: i32, out_dev: *mut u8, out_cap: i64, out_len: *mut i32, status: *mut i32, offset: *mut i64,
                               f_delta: *mut f64, metric: *mut f32) -> c_int;
    pub fn ofdm_rx_decode_long_host(ctx: *mut ofdm_ctx, in_host: *const ofdm_fc32, n_samples: i64, max_symbols: i32, out_host: *mut u8,
                                    out_cap: i64, out_len: *mut i32, status: *mut i32, offset: *mut i64, f_delta: *mut f64,
                                    metric: *mut f32) -> c_int;
    // EXT-12: every detection of a lag range under the holdoff rule (include/ofdm_hip.h); d1, f_delta, metric and more may be null
    pub fn ofdm_sc_scan_long(ctx: *mut ofdm_ctx, in_dev: *const ofdm_fc32, n_samples: i64, lag_lo: i64, lag_hi: i64, holdoff: i64, max_det: i64,
                             d1: *mut i64, d_hat: *mut i64, f_delta: *mut f64, metric: *mut f32, n_det: *mut i64, more: *mut i32) -> c_int;
    pub fn ofdm_sc_scan_long_host(ctx: *mut ofdm_ctx, in_host: *const ofdm_fc32, n_samples: i64, lag_lo: i64, lag_hi: i64, holdoff: i64,
                                  max_det: i64, d1: *mut i64, d_hat: *mut i64, f_delta: *mut f64, metric: *mut f32, n_det: *mut i64,
                                  more: *mut i32) -> c_int;
    // EXT-13: every packet of one long capture in ONE run of the receive chain, from the scan's (d_hat, f_delta, metric) triples (host
    // arrays); outputs on the device, offset / f_delta / metric may be null.  _all_long_host: upload + scan + decode into host arrays
    pub fn ofdm_rx_decode_packets(ctx: *mut ofdm_ctx, in_dev: *const ofdm_fc32, n_samples: i64, n_det: i64, d_hat: *const i64, f_delta: *const f64,
                                  metric: *const f32, max_symbols: i32, out_dev: *mut u8, out_stride: i64, out_len_dev: *mut i32,
                                  status_dev: *mut i32, offset_dev: *mut i64, f_delta_dev: *mut f64, metric_dev: *mut f32) -> c_int;
    pub fn ofdm_rx_decode_all_long_host(ctx: *mut ofdm_ctx, in_host: *const ofdm_fc32, n_samples: i64, lag_lo: i64, lag_hi: i64, holdoff: i64,
                                        max_det: i64, max_symbols: i32, out_host: *mut u8, out_stride: i64, out_len: *mut i32,
                                        status: *mut i32, offset: *mut i64, f_delta: *mut f64, metric: *mut f32, d1: *mut i64,
                                        d_hat: *mut i64, n_det: *mut i64, more: *mut i32) -> c_int;
    pub fn ofdm_sc16_widen(input: *const ofdm_sc16, n: i64, scale: f32, out: *mut ofdm_fc32) -> c_int;
    pub fn ofdm_sc16_narrow(input: *const ofdm_fc32, n: i64, scale: f32, out: *mut ofdm_sc16, clipped: *mut i64) -> c_int;
    pub fn ofdm_sc16_widen_batch(ctx: *mut ofdm_ctx, in_dev: *const ofdm_sc16, n_frames: i64, in_stride: i64, frame_len: i64, scale: f32,
                                 out_dev: *mut ofdm_fc32, out_stride: i64) -> c_int;
    pub fn ofdm_sc16_narrow_batch(ctx: *mut ofdm_ctx, in_dev: *const ofdm_fc32, n_frames: i64, in_stride: i64, frame_len: i64, scale: f32,
                                  out_dev: *mut ofdm_sc16, out_stride: i64, clipped_dev: *mut i32) -> c_int;
    pub fn ofdm_rx_demod_sc16_batch(ctx: *mut ofdm_ctx, in_dev: *const ofdm_sc16, n_frames: i64, frame_stride: i64, frame_len: i64, scale: f32,
                                    first_symbol: i32, syms_per_frame: i32, offset_dev: *const i32, f_delta_dev: *const f64,
                                    hk_dev: *const ofdm_fc32, hk_stride: i64, out_dev: *mut u8, out_stride: i64, soft_dev: *mut ofdm_fc32) -> c_int;
    pub fn ofdm_rx_decode_sc16_batch(ctx: *mut ofdm_ctx, in_dev: *const ofdm_sc16, n_frames: i64, frame_stride: i64, frame_len: i64, scale: f32,
                                     n_lags: i64, max_symbols: i32, out_dev: *mut u8, out_stride: i64, out_len_dev: *mut i32,
                                     status_dev: *mut i32, offset_dev: *mut i32, f_delta_dev: *mut f64, metric_dev: *mut f32) -> c_int;
    pub fn ofdm_rx_demod_sc16_host(ctx: *mut ofdm_ctx, in_host: *const ofdm_sc16, n_frames: i64, frame_stride: i64, frame_len: i64, scale: f32,
                                   first_symbol: i32, syms_per_frame: i32, out_host: *mut u8, out_stride: i64, chunk_frames: i64) -> c_int;
    pub fn ofdm_rx_decode_sc16_host(ctx: *mut ofdm_ctx, in_host: *const ofdm_sc16, n_frames: i64, frame_stride: i64, frame_len: i64, scale: f32,
                                    n_lags: i64, max_symbols: i32, out_host: *mut u8, out_stride: i64, out_len_host: *mut i32,
                                    status_host: *mut i32, offset_host: *mut i32, f_delta_host: *mut f64, metric_host: *mut f32,
                                    chunk_frames: i64) -> c_int;
    // EXT-10: sc16 transmit output (clipped_*: optional, int32 per frame) and sc16 long captures
    pub fn ofdm_tx_encode_sc16_batch(ctx: *mut ofdm_ctx, payload_dev: *const u8, n_frames: i64, payload_stride: i64, payload_len_dev: *const i32,
                                     payload_bytes: i32, scale: f32, out_dev: *mut ofdm_sc16, out_stride: i64, clipped_dev: *mut i32) -> c_int;
    pub fn ofdm_tx_encode_sc16_host(ctx: *mut ofdm_ctx, payload_host: *const u8, n_frames: i64, payload_stride: i64, payload_len_host: *const i32,
                                    payload_bytes: i32, scale: f32, out_host: *mut ofdm_sc16, out_stride: i64, clipped_host: *mut i32,
                                    chunk_frames: i64) -> c_int;
    pub fn ofdm_rx_decode_long_sc16(ctx: *mut ofdm_ctx, in_dev: *const ofdm_sc16, n_samples: i64, scale: f32, lag_lo: i64, lag_hi: i64,
                                    d_hat_known: i64, max_symbols: i32, out_dev: *mut u8, out_cap: i64, out_len: *mut i32, status: *mut i32,
                                    offset: *mut i64, f_delta: *mut f64, metric: *mut f32) -> c_int;
    pub fn ofdm_rx_decode_long_sc16_host(ctx: *mut ofdm_ctx, in_host: *const ofdm_sc16, n_samples: i64, scale: f32, max_symbols: i32,
                                         out_host: *mut u8, out_cap: i64, out_len: *mut i32, status: *mut i32, offset: *mut i64,
                                         f_delta: *mut f64, metric: *mut f32) -> c_int;
    // EXT-14: a streaming receiver.  The handle comes first (create: its address, then the context); offset, d1 and more may be null
    pub fn ofdm_stream_create(out: *mut *mut ofdm_stream, ctx: *mut ofdm_ctx, max_symbols: i32, holdoff: i64, max_chunk: i64,
                              first_sample: i64) -> c_int;
    pub fn ofdm_stream_destroy(s: *mut ofdm_stream) -> c_int;
    pub fn ofdm_stream_reset(s: *mut ofdm_stream, first_sample: i64) -> c_int;
    pub fn ofdm_stream_push(s: *mut ofdm_stream, in_host: *const ofdm_fc32, n: i64, flush: i32, max_pkt: i64, out_host: *mut u8, out_stride: i64,
                            out_len: *mut i32, status: *mut i32, offset: *mut i64, f_delta: *mut f64, metric: *mut f32, d1: *mut i64,
                            d_hat: *mut i64, n_pkt: *mut i64, more: *mut i32) -> c_int;
    pub fn ofdm_stream_push_sc16(s: *mut ofdm_stream, in_host: *const ofdm_sc16, n: i64, scale: f32, flush: i32, max_pkt: i64, out_host: *mut u8,
                                 out_stride: i64, out_len: *mut i32, status: *mut i32, offset: *mut i64, f_delta: *mut f64, metric: *mut f32,
                                 d1: *mut i64, d_hat: *mut i64, n_pkt: *mut i64, more: *mut i32) -> c_int;
    pub fn ofdm_stream_state(s: *const ofdm_stream, total: *mut i64, kept_from: *mut i64, next_lag: *mut i64, ended: *mut i32) -> c_int;
    // EXT-15: a DC blocker.  Host definition; a handle on device buffers (its own type first); the stream option
    pub fn ofdm_dc_block_default(n_fft: i32, cp_len: i32) -> c_int;
    pub fn ofdm_dc_block(input: *const ofdm_fc32, n: i64, blocks: i32, out: *mut ofdm_fc32) -> c_int;
    pub fn ofdm_dc_block_sc16(input: *const ofdm_sc16, n: i64, scale: f32, blocks: i32, out: *mut ofdm_fc32) -> c_int;
    pub fn ofdm_dcblock_create(out: *mut *mut ofdm_dcblock, ctx: *mut ofdm_ctx, blocks: i32, max_chunk: i64) -> c_int;
    pub fn ofdm_dcblock_destroy(f: *mut ofdm_dcblock) -> c_int;
    pub fn ofdm_dcblock_reset(f: *mut ofdm_dcblock) -> c_int;
    pub fn ofdm_dcblock_push(f: *mut ofdm_dcblock, in_dev: *const ofdm_fc32, n: i64, out_dev: *mut ofdm_fc32) -> c_int;
    pub fn ofdm_dcblock_push_sc16(f: *mut ofdm_dcblock, in_dev: *const ofdm_sc16, n: i64, scale: f32, out_dev: *mut ofdm_fc32) -> c_int;
    pub fn ofdm_dcblock_state(f: *const ofdm_dcblock, total: *mut i64, blocks: *mut i32) -> c_int;
    pub fn ofdm_stream_set_dc_block(s: *mut ofdm_stream, blocks: i32) -> c_int;
    pub fn ofdm_stream_get_dc_block(s: *const ofdm_stream, blocks: *mut i32) -> c_int;
    // EXT-16: a digital down-converter.  Host definition and design; a handle on device buffers (its own type first); the stream option
    pub fn ofdm_ddc_rotor_tables(coarse: *mut f32, fine: *mut f32) -> c_int;
    pub fn ofdm_ddc_out_len(n: i64, decim: i32, n_taps: i32) -> i64;
    pub fn ofdm_ddc_inc_for(f0_cycles_per_sample: f64, inc: *mut i32) -> c_int;
    pub fn ofdm_ddc_design(decim: i32, taps_per_phase: i32, taps: *mut f32) -> c_int;
    pub fn ofdm_ddc(input: *const ofdm_fc32, n: i64, decim: i32, phase_inc: i32, taps: *const f32, n_taps: i32, out: *mut ofdm_fc32,
                    out_cap: i64, n_out: *mut i64) -> c_int;
    pub fn ofdm_ddc_sc16(input: *const ofdm_sc16, n: i64, scale: f32, decim: i32, phase_inc: i32, taps: *const f32, n_taps: i32,
                         out: *mut ofdm_fc32, out_cap: i64, n_out: *mut i64) -> c_int;
    pub fn ofdm_ddc_create(out: *mut *mut ofdm_ddc_handle, ctx: *mut ofdm_ctx, decim: i32, phase_inc: i32, taps: *const f32, n_taps: i32,
                           max_chunk: i64) -> c_int;
    pub fn ofdm_ddc_destroy(h: *mut ofdm_ddc_handle) -> c_int;
    pub fn ofdm_ddc_reset(h: *mut ofdm_ddc_handle) -> c_int;
    pub fn ofdm_ddc_push(h: *mut ofdm_ddc_handle, in_dev: *const ofdm_fc32, n: i64, out_dev: *mut ofdm_fc32, out_cap: i64, n_out: *mut i64) -> c_int;
    pub fn ofdm_ddc_push_sc16(h: *mut ofdm_ddc_handle, in_dev: *const ofdm_sc16, n: i64, scale: f32, out_dev: *mut ofdm_fc32, out_cap: i64,
                              n_out: *mut i64) -> c_int;
    pub fn ofdm_ddc_state(h: *const ofdm_ddc_handle, total_in: *mut i64, total_out: *mut i64) -> c_int;
    pub fn ofdm_stream_set_ddc(s: *mut ofdm_stream, decim: i32, phase_inc: i32, taps: *const f32, n_taps: i32) -> c_int;
    pub fn ofdm_stream_get_ddc(s: *const ofdm_stream, decim: *mut i32, phase_inc: *mut i32, n_taps: *mut i32) -> c_int;
    pub fn ofdm_timer_start(ctx: *mut ofdm_ctx) -> c_int;
    pub fn ofdm_timer_stop_ms(ctx: *mut ofdm_ctx, elapsed_ms: *mut f32) -> c_int;
}

/// Owning wrapper: one context per (thread, GPU).
pub struct Ctx { raw: *mut ofdm_ctx, s: usize, bytes_per_symbol: usize }

fn check(rc: c_int, what: &str) -> anyhow::Result<()> {
    if rc == OFDM_OK { Ok(()) } else {
        let msg = unsafe { std::ffi::CStr::from_ptr(ofdm_strerror(rc)) }.to_string_lossy().into_owned();
        Err(anyhow::anyhow!("{}: {}", what, msg))
    }
}

impl Ctx {
    pub fn new(guard_bands: bool, modulation: i32) -> anyhow::Result<Self> { Self::on_device(guard_bands, modulation, 0) }
    pub fn on_device(guard_bands: bool, modulation: i32, device: i32) -> anyhow::Result<Self> {
        let mut p: ofdm_params = unsafe { std::mem::zeroed() };
        check(unsafe { ofdm_default_params(&mut p) }, "ofdm_default_params")?;
        p.guard_bands = guard_bands as i32;
        p.modulation = modulation;
        let mut raw = std::ptr::null_mut();
        check(unsafe { ofdm_create(&p, std::ptr::null(), std::ptr::null(), device, std::ptr::null_mut(), &mut raw) }, "ofdm_create")?;
        let s = unsafe { ofdm_symbol_len(raw) } as usize;
        let bps = unsafe { ofdm_bytes_per_symbol(raw) } as usize;
        Ok(Ctx { raw, s, bytes_per_symbol: bps })
    }
    fn alloc(&self, bytes: usize) -> anyhow::Result<*mut c_void> {
        let mut d = std::ptr::null_mut();
        check(unsafe { ofdm_dev_alloc(self.raw, bytes, &mut d) }, "ofdm_dev_alloc")?;
        Ok(d)
    }
}
impl Drop for Ctx { fn drop(&mut self) { unsafe { ofdm_destroy(self.raw); } } }

/// EXT-14: a streaming receiver on a context (include/ofdm_hip.h, "a streaming receiver").  `push` takes the samples as a radio hands them
/// over and returns the packets that push made deliverable; however the stream is cut they are, bit for bit, the packets of one
/// `ofdm_rx_decode_all_long_host` call on the concatenation, each exactly once.  Borrows its context, so it is dropped before it.
pub struct StreamPacket { pub bytes: Vec<u8>, pub status: i32, pub offset: i64, pub d1: i64, pub d_hat: i64, pub f_delta: f64, pub metric: f32 }
pub struct Stream<'a> { raw: *mut ofdm_stream, row: usize, _ctx: std::marker::PhantomData<&'a Ctx> }
impl<'a> Stream<'a> {
    pub fn new(ctx: &'a Ctx, max_symbols: i32, holdoff: i64, max_chunk: i64, first_sample: i64) -> anyhow::Result<Self> {
        let mut raw = std::ptr::null_mut();
        check(unsafe { ofdm_stream_create(&mut raw, ctx.raw, max_symbols, holdoff, max_chunk, first_sample) }, "ofdm_stream_create")?;
        Ok(Stream { raw, row: (max_symbols as usize * ctx.bytes_per_symbol).max(4) + 256, _ctx: std::marker::PhantomData })
    }
    /// `samples` (may be empty), then everything drained through `more`; `flush` ends the stream until `reset`
    pub fn push(&mut self, samples: &[ofdm_fc32], flush: bool) -> anyhow::Result<Vec<StreamPacket>> {
        const BATCH: usize = 64;
        let mut out = Vec::new();
        let mut rows = vec![0u8; BATCH * self.row];
        let (mut len, mut status, mut offset, mut d1, mut d_hat) = ([0i32; BATCH], [0i32; BATCH], [0i64; BATCH], [0i64; BATCH], [0i64; BATCH]);
        let (mut f_delta, mut metric, mut n, mut more) = ([0f64; BATCH], [0f32; BATCH], 0i64, 0i32);
        let mut first = true;
        loop {
            let (p, k) = if first { (samples.as_ptr(), samples.len() as i64) } else { (std::ptr::null(), 0) };
            check(unsafe { ofdm_stream_push(self.raw, p, k, flush as i32, BATCH as i64, rows.as_mut_ptr(), self.row as i64, len.as_mut_ptr(),
                                            status.as_mut_ptr(), offset.as_mut_ptr(), f_delta.as_mut_ptr(), metric.as_mut_ptr(), d1.as_mut_ptr(),
                                            d_hat.as_mut_ptr(), &mut n, &mut more) }, "ofdm_stream_push")?;
            first = false;
            for i in 0..n as usize {
                let bytes = if status[i] == 0 && len[i] > 0 { rows[i * self.row..i * self.row + len[i] as usize].to_vec() } else { Vec::new() };
                out.push(StreamPacket { bytes, status: status[i], offset: offset[i], d1: d1[i], d_hat: d_hat[i], f_delta: f_delta[i], metric: metric[i] });
            }
            if more == 0 { return Ok(out); }
        }
    }
    pub fn flush(&mut self) -> anyhow::Result<Vec<StreamPacket>> { self.push(&[], true) }
    pub fn reset(&mut self, first_sample: i64) -> anyhow::Result<()> { check(unsafe { ofdm_stream_reset(self.raw, first_sample) }, "ofdm_stream_reset") }
    /// EXT-15: the DC blocker in front of the window (0 = off); only before the first sample or right after `reset`, which keeps the setting
    pub fn set_dc_block(&mut self, blocks: i32) -> anyhow::Result<()> { check(unsafe { ofdm_stream_set_dc_block(self.raw, blocks) }, "ofdm_stream_set_dc_block") }
    pub fn dc_block(&self) -> anyhow::Result<i32> {
        let mut m = 0i32;
        check(unsafe { ofdm_stream_get_dc_block(self.raw, &mut m) }, "ofdm_stream_get_dc_block")?;
        Ok(m)
    }
    /// EXT-16: the down-converter in front of everything else (decim 0 = off; empty taps: the default design).  Pushes are then
    /// input-rate samples, every offset is in output samples; only before the first sample or right after `reset`
    pub fn set_ddc(&mut self, decim: i32, phase_inc: i32, taps: &[f32]) -> anyhow::Result<()> {
        let p = if taps.is_empty() { std::ptr::null() } else { taps.as_ptr() };
        check(unsafe { ofdm_stream_set_ddc(self.raw, decim, phase_inc, p, taps.len() as i32) }, "ofdm_stream_set_ddc")
    }
    /// (decim, phase_inc, n_taps) of the setting; decim 0 = off
    pub fn ddc(&self) -> anyhow::Result<(i32, i32, i32)> {
        let (mut d, mut i, mut t) = (0i32, 0i32, 0i32);
        check(unsafe { ofdm_stream_get_ddc(self.raw, &mut d, &mut i, &mut t) }, "ofdm_stream_get_ddc")?;
        Ok((d, i, t))
    }
}
impl<'a> Drop for Stream<'a> { fn drop(&mut self) { unsafe { ofdm_stream_destroy(self.raw); } } }

/// EXT-16: a digital down-converter on device buffers (include/ofdm_hip.h, "a digital down-converter"): mix by the two-level 20-bit
/// rotor, filter by real taps, keep every `decim`-th sample; the outputs of one converter's pushes, concatenated, equal `ofdm_ddc` of the
/// concatenated inputs bit for bit.  `input` and `out` are device pointers that do not overlap.  Borrows its context.
pub struct Ddc<'a> { raw: *mut ofdm_ddc_handle, _ctx: std::marker::PhantomData<&'a Ctx> }
impl<'a> Ddc<'a> {
    pub fn new(ctx: &'a Ctx, decim: i32, phase_inc: i32, taps: &[f32], max_chunk: i64) -> anyhow::Result<Self> {
        let mut raw = std::ptr::null_mut();
        check(unsafe { ofdm_ddc_create(&mut raw, ctx.raw, decim, phase_inc, taps.as_ptr(), taps.len() as i32, max_chunk) }, "ofdm_ddc_create")?;
        Ok(Ddc { raw, _ctx: std::marker::PhantomData })
    }
    /// -> the samples written at `out`
    pub unsafe fn push(&mut self, input: *const ofdm_fc32, n: i64, out: *mut ofdm_fc32, out_cap: i64) -> anyhow::Result<i64> {
        let mut k = 0i64;
        check(ofdm_ddc_push(self.raw, input, n, out, out_cap, &mut k), "ofdm_ddc_push")?;
        Ok(k)
    }
    pub unsafe fn push_sc16(&mut self, input: *const ofdm_sc16, n: i64, scale: f32, out: *mut ofdm_fc32, out_cap: i64) -> anyhow::Result<i64> {
        let mut k = 0i64;
        check(ofdm_ddc_push_sc16(self.raw, input, n, scale, out, out_cap, &mut k), "ofdm_ddc_push_sc16")?;
        Ok(k)
    }
    pub fn reset(&mut self) -> anyhow::Result<()> { check(unsafe { ofdm_ddc_reset(self.raw) }, "ofdm_ddc_reset") }
    /// (samples taken, samples given) since create / reset
    pub fn state(&self) -> anyhow::Result<(i64, i64)> {
        let (mut a, mut b) = (0i64, 0i64);
        check(unsafe { ofdm_ddc_state(self.raw, &mut a, &mut b) }, "ofdm_ddc_state")?;
        Ok((a, b))
    }
}
impl<'a> Drop for Ddc<'a> { fn drop(&mut self) { unsafe { ofdm_ddc_destroy(self.raw); } } }
/// The Hamming-windowed sinc of `taps_per_phase * decim` taps with the cutoff 0.5 / decim (`ofdm_ddc_design`)
pub fn ddc_design(decim: i32, taps_per_phase: i32) -> anyhow::Result<Vec<f32>> {
    let mut h = vec![0f32; (decim.max(1) as usize) * (taps_per_phase.max(1) as usize)];
    check(unsafe { ofdm_ddc_design(decim, taps_per_phase, h.as_mut_ptr()) }, "ofdm_ddc_design")?;
    Ok(h)
}
/// The increment that brings `f0` (cycles per input sample) to 0 (`ofdm_ddc_inc_for`)
pub fn ddc_inc_for(f0: f64) -> anyhow::Result<i32> {
    let mut inc = 0i32;
    check(unsafe { ofdm_ddc_inc_for(f0, &mut inc) }, "ofdm_ddc_inc_for")?;
    Ok(inc)
}
/// The rotor tables the host definition uses and the device is given (`ofdm_ddc_rotor_tables`): 1024 (re, im) pairs each
pub fn ddc_rotor_tables() -> anyhow::Result<(Vec<f32>, Vec<f32>)> {
    let (mut c, mut f) = (vec![0f32; 2048], vec![0f32; 2048]);
    check(unsafe { ofdm_ddc_rotor_tables(c.as_mut_ptr(), f.as_mut_ptr()) }, "ofdm_ddc_rotor_tables")?;
    Ok((c, f))
}
/// The definition on host slices, no GPU (`ofdm_ddc` / `ofdm_ddc_sc16`)
pub fn ddc_host(samples: &[ofdm_fc32], decim: i32, phase_inc: i32, taps: &[f32]) -> anyhow::Result<Vec<ofdm_fc32>> {
    let m = unsafe { ofdm_ddc_out_len(samples.len() as i64, decim, taps.len() as i32) };
    check(if m < 0 { m as c_int } else { 0 }, "ofdm_ddc_out_len")?;
    let mut out: Vec<ofdm_fc32> = Vec::with_capacity(m as usize);
    let mut k = 0i64;
    check(unsafe { ofdm_ddc(samples.as_ptr(), samples.len() as i64, decim, phase_inc, taps.as_ptr(), taps.len() as i32, out.as_mut_ptr(), m, &mut k) }, "ofdm_ddc")?;
    unsafe { out.set_len(k as usize); }
    Ok(out)
}
pub fn ddc_sc16_host(samples: &[ofdm_sc16], scale: f32, decim: i32, phase_inc: i32, taps: &[f32]) -> anyhow::Result<Vec<ofdm_fc32>> {
    let m = unsafe { ofdm_ddc_out_len(samples.len() as i64, decim, taps.len() as i32) };
    check(if m < 0 { m as c_int } else { 0 }, "ofdm_ddc_out_len")?;
    let mut out: Vec<ofdm_fc32> = Vec::with_capacity(m as usize);
    let mut k = 0i64;
    check(unsafe { ofdm_ddc_sc16(samples.as_ptr(), samples.len() as i64, scale, decim, phase_inc, taps.as_ptr(), taps.len() as i32, out.as_mut_ptr(), m, &mut k) }, "ofdm_ddc_sc16")?;
    unsafe { out.set_len(k as usize); }
    Ok(out)
}

/// EXT-15: a DC blocker on device buffers (include/ofdm_hip.h, "a DC blocker in front of detection").  Every sample leaves less the mean of
/// the `blocks` complete 64-sample blocks in front of its own block; the pushes of one filter, concatenated, equal `ofdm_dc_block` of the
/// concatenated inputs bit for bit.  `input` and `out` are device pointers that do not overlap.  Borrows its context.
pub struct DcBlock<'a> { raw: *mut ofdm_dcblock, _ctx: std::marker::PhantomData<&'a Ctx> }
impl<'a> DcBlock<'a> {
    /// `blocks` 0: `ofdm_dc_block_default` of the context's own sizes (S = n_fft + n_fft / 4)
    pub fn new(ctx: &'a Ctx, blocks: i32, max_chunk: i64) -> anyhow::Result<Self> {
        let n_fft = (ctx.s * 4 / 5) as i32;
        let m = if blocks != 0 { blocks } else { unsafe { ofdm_dc_block_default(n_fft, n_fft / 4) } };
        let mut raw = std::ptr::null_mut();
        check(unsafe { ofdm_dcblock_create(&mut raw, ctx.raw, m, max_chunk) }, "ofdm_dcblock_create")?;
        Ok(DcBlock { raw, _ctx: std::marker::PhantomData })
    }
    pub unsafe fn push(&mut self, input: *const ofdm_fc32, n: i64, out: *mut ofdm_fc32) -> anyhow::Result<()> {
        check(ofdm_dcblock_push(self.raw, input, n, out), "ofdm_dcblock_push")
    }
    pub unsafe fn push_sc16(&mut self, input: *const ofdm_sc16, n: i64, scale: f32, out: *mut ofdm_fc32) -> anyhow::Result<()> {
        check(ofdm_dcblock_push_sc16(self.raw, input, n, scale, out), "ofdm_dcblock_push_sc16")
    }
    pub fn reset(&mut self) -> anyhow::Result<()> { check(unsafe { ofdm_dcblock_reset(self.raw) }, "ofdm_dcblock_reset") }
    /// (samples pushed since create / reset, blocks)
    pub fn state(&self) -> anyhow::Result<(i64, i32)> {
        let (mut t, mut m) = (0i64, 0i32);
        check(unsafe { ofdm_dcblock_state(self.raw, &mut t, &mut m) }, "ofdm_dcblock_state")?;
        Ok((t, m))
    }
}
impl<'a> Drop for DcBlock<'a> { fn drop(&mut self) { unsafe { ofdm_dcblock_destroy(self.raw); } } }
/// The definition on host slices, no GPU (`ofdm_dc_block` / `ofdm_dc_block_sc16`)
pub fn dc_block_host(samples: &[ofdm_fc32], blocks: i32) -> anyhow::Result<Vec<ofdm_fc32>> {
    let mut out: Vec<ofdm_fc32> = Vec::with_capacity(samples.len());
    check(unsafe { ofdm_dc_block(samples.as_ptr(), samples.len() as i64, blocks, out.as_mut_ptr()) }, "ofdm_dc_block")?;
    unsafe { out.set_len(samples.len()); }
    Ok(out)
}
pub fn dc_block_sc16_host(samples: &[ofdm_sc16], scale: f32, blocks: i32) -> anyhow::Result<Vec<ofdm_fc32>> {
    let mut out: Vec<ofdm_fc32> = Vec::with_capacity(samples.len());
    check(unsafe { ofdm_dc_block_sc16(samples.as_ptr(), samples.len() as i64, scale, blocks, out.as_mut_ptr()) }, "ofdm_dc_block_sc16")?;
    unsafe { out.set_len(samples.len()); }
    Ok(out)
}

/// One context per (thread, parameter set), created on first use and kept for the life of the thread: the reference calls `encode!` /
/// `decode!` once per frame (examples/lab3a.rs:24,34, jetson_rx.rs:86) and `ofdm_create` -- table uploads, streams, workspaces --
/// must not be paid on every call (round 3 did: 1.6 ms per call against 0.1 ms for the decode itself).
thread_local! {
    static CTX_CACHE: std::cell::RefCell<std::collections::HashMap<(bool, i32), std::rc::Rc<Ctx>>> = Default::default();
}
fn ctx_for(guard_bands: bool, modulation: i32) -> anyhow::Result<std::rc::Rc<Ctx>> {
    CTX_CACHE.with(|c| {
        let mut c = c.borrow_mut();
        if let Some(x) = c.get(&(guard_bands, modulation)) { return Ok(x.clone()); }
        let x = std::rc::Rc::new(Ctx::new(guard_bands, modulation)?);
        c.insert((guard_bands, modulation), x.clone());
        Ok(x)
    })
}

/// `ofdm::encode!(data, guard_bands, modulation)` -- the reference's exact signature (src/transmitter.rs:10-15), so the
/// `#[optargs::optfn]` attribute and every `encode!` call site stay as they are.  The reference cannot fail here; a GPU can
/// (no device, out of memory): like the reference's own `unwrap`s this panics rather than change the return type.
#[optargs::optfn]
pub fn encode(data: &[u8], guard_bands: Option<bool>, modulation: Option<crate::ModulationScheme>) -> Vec<Complex64> {
    try_encode(data, guard_bands, modulation).expect("ofdm_hip encode")
}

/// Fallible form for hosts that prefer a `Result` over the panic.  Host bytes in, host samples out: `ofdm_tx_encode_host` stages
/// through the library's pinned buffers (no device allocation per call).
pub fn try_encode(data: &[u8], guard_bands: Option<bool>, modulation: Option<crate::ModulationScheme>) -> anyhow::Result<Vec<Complex64>> {
    let ctx = ctx_for(guard_bands.unwrap_or(false), bits_per_point(&modulation.unwrap_or(ModulationScheme::Bpsk)))?;
    let n = unsafe { ofdm_frame_samples(ctx.raw, data.len() as i64) } as usize;
    let mut host = vec![ofdm_fc32 { re: 0.0, im: 0.0 }; n];
    let none = [0u8];
    let src = if data.is_empty() { none.as_ptr() } else { data.as_ptr() };
    check(unsafe { ofdm_tx_encode_host(ctx.raw, src, 1, data.len() as i64, std::ptr::null(), data.len() as i32, host.as_mut_ptr(), n as i64, 0) },
          "ofdm_tx_encode_host")?;
    Ok(host.iter().map(|c| Complex64::new(c.re as f64, c.im as f64)).collect()) // bytes_to_sig, src/utils.rs:238-254
}

/// `ofdm::decode!(samples, guard_bands, modulation)` -- the reference's exact signature (src/receiver.rs:8-13).  ONE capture of any
/// length: the 2 M-sample buffers of examples/jetson_rx.rs:15-17,84-86 are searched as a batch of overlapping slices
/// (`ofdm_rx_decode_long_host`), a frame-sized capture takes the batch path directly.
#[optargs::optfn]
pub fn decode(samples: Vec<Complex64>, guard_bands: Option<bool>, modulation: Option<crate::ModulationScheme>) -> anyhow::Result<Vec<u8>> {
    let ctx = ctx_for(guard_bands.unwrap_or(false), bits_per_point(&modulation.unwrap_or(ModulationScheme::Bpsk)))?;
    let n = samples.len();
    let fc32: Vec<ofdm_fc32> = samples.iter().map(|c| ofdm_fc32 { re: c.re as f32, im: c.im as f32 }).collect(); // sig_to_bytes
    let max_sym = (((n + ctx.s - 1) / ctx.s).saturating_sub(10)).max(1);
    let cap = (max_sym * ctx.bytes_per_symbol).max(4);
    let mut bytes = vec![0u8; cap];
    let (mut len, mut status, mut offset) = (0i32, 0i32, 0i64);
    check(unsafe { ofdm_rx_decode_long_host(ctx.raw, fc32.as_ptr(), n as i64, max_sym as i32, bytes.as_mut_ptr(), cap as i64, &mut len, &mut status,
                                            &mut offset, std::ptr::null_mut(), std::ptr::null_mut()) }, "ofdm_rx_decode_long_host")?;
    match status {
        0 => { bytes.truncate(len as usize); Ok(bytes) }
        OFDM_FRAME_SHORT => Err(anyhow::anyhow!("Input not long enough, bailing early")),
        s => Err(anyhow::anyhow!("decode failed (frame status {})", s)),
    }
}

/// Frame-index data parallelism inside one process (the C++ twin is `ofdm::ShardedContext` in include/ofdm_host.hpp):
/// one context per entry of `devices` (an ordinal may repeat), each with its own stream (`ofdm_use_own_stream`), one scoped thread per
/// context for the duration of a call, frames [r F / R, (r + 1) F / R) to context r, results written straight into the caller's
/// arrays -- no exchange between the devices.  `Ctx` is `Send` (a context may move between threads; it must not be shared).
pub struct ShardedCtx { ctxs: Vec<Ctx> }
unsafe impl Send for Ctx {}
impl ShardedCtx {
    pub fn new(devices: &[i32], guard_bands: bool, modulation: i32) -> anyhow::Result<Self> {
        let mut ctxs = Vec::new();
        for &d in devices {
            let c = Ctx::on_device(guard_bands, modulation, d)?;
            check(unsafe { ofdm_use_own_stream(c.raw) }, "ofdm_use_own_stream")?;
            ctxs.push(c);
        }
        Ok(ShardedCtx { ctxs })
    }
    /// decode_batch on host memory: `frames` holds n_frames rows of `stride` fc32 samples; returns (bytes rows of `row` bytes, len, status)
    pub fn decode_batch(&mut self, frames: &[ofdm_fc32], n_frames: usize, stride: usize, max_symbols: i32) -> anyhow::Result<(Vec<u8>, usize, Vec<i32>, Vec<i32>)> {
        let row = ((max_symbols as usize) * self.ctxs[0].bytes_per_symbol).saturating_sub(16).max(4);
        let (mut bytes, mut len, mut status) = (vec![0u8; n_frames * row], vec![0i32; n_frames], vec![0i32; n_frames]);
        let r = self.ctxs.len();
        let rcs: Vec<c_int> = std::thread::scope(|sc| {
            let mut hs = Vec::new();
            let (mut b, mut l, mut s) = (&mut bytes[..], &mut len[..], &mut status[..]);
            for (i, c) in self.ctxs.iter_mut().enumerate() {
                let (lo, hi) = (n_frames * i / r, n_frames * (i + 1) / r);
                let (bi, br) = b.split_at_mut((hi - lo) * row); b = br;
                let (li, lr) = l.split_at_mut(hi - lo); l = lr;
                let (si, sr) = s.split_at_mut(hi - lo); s = sr;
                let src = &frames[lo * stride..];
                hs.push(sc.spawn(move || unsafe {
                    ofdm_rx_decode_host(c.raw, src.as_ptr(), (hi - lo) as i64, stride as i64, stride as i64, 0, max_symbols, bi.as_mut_ptr(), row as i64,
                                        li.as_mut_ptr(), si.as_mut_ptr(), std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut(), 0)
                }));
            }
            hs.into_iter().map(|h| h.join().unwrap()).collect()
        });
        for rc in rcs { check(rc, "ofdm_rx_decode_host")?; }
        Ok((bytes, row, len, status))
    }
}
