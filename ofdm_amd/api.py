"""Host-side mirror of the reference's TX/RX function surface over the C ABI (include/ofdm_hip.h).

The reference's hot path is a set of free functions re-exported from its crate root (src/lib.rs:8-21):
`encode`, `decode`, `modulate`, `demodulate`, `encode_block`, `prefix_block`, `unprefix_block`,
`estimate_channel`, `frequency_correction`, `normalize`, `locking_signal`, `preamble`, `training_signals`.
This module keeps those names, argument meanings, defaults and error behaviour, batch-first, with the DSP
bodies running as HIP kernels on one MI355X.  torch is used for device memory and streams only: every
computation goes through libofdm_hip.so, and nothing here falls back to the CPU.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib

BPSK, QPSK, QAM16, QAM64, QAM256 = 1, 2, 4, 6, 8  # ModulationScheme (src/transmitter.rs:98-104) as bits/point
ECC_NONE, ECC_HAMMING74, ECC_HAMMING74_SOFT = 0, 1, 2
ECC_CONV_K7 = 5  # K = 7 rate-1/2 convolutional code, Viterbi-decoded from LLRs (3 and 4 are not modes)
# framed convolutional modes: a coded length block in front of the payload at rate 1/2, 2/3, 3/4 (tests/framed_ref.py is the definition)
ECC_CONV_K7F_R12, ECC_CONV_K7F_R23, ECC_CONV_K7F_R34 = 10, 11, 12
# outer Reed-Solomon(255,223) around the frames of an inner mode, 20 + inner (inner = ECC_NONE or a framed mode): the reference's
# create_transmission_bytes / decipher_transmission_bytes inside encode / decode, on the device
ECC_RS255, ECC_RS255_K7F_R12, ECC_RS255_K7F_R23, ECC_RS255_K7F_R34 = 20, 30, 31, 32
# CRC-32 frame check around any mode (the LDPC modes below included), 64 + mode: decode delivers exactly the payload that was sent or reports the
# frame with FRAME_FCS (tests/fcs_ref.py is the definition)
ECC_FCS = 64
# LDPC(648,324), rate 1/2, layered min-sum from LLRs; the length travels in the first code word (tests/ldpc_ref.py is the definition)
ECC_LDPC648 = 16
# the project's own LDPC(648) codes of rates 2/3, 3/4 and 5/6 under the same frame rule, K = 53 / 60 / 67 info bytes to 80 coded bytes
# (tests/ldpc_rates_ref.py is the definition); `rate=` of Context.ldpc_encode / ldpc_decode: 0 = 1/2, 1 = 2/3, 2 = 3/4, 3 = 5/6
ECC_LDPC648_R23, ECC_LDPC648_R34, ECC_LDPC648_R56 = 41, 42, 43
LDPC_RATE_1_2, LDPC_RATE_2_3, LDPC_RATE_3_4, LDPC_RATE_5_6 = 0, 1, 2, 3
LDPC_INFO_BYTES = (40, 53, 60, 67)  # ofdm_ldpc648_info_bytes(rate)
LDPC_MAX_ITER = 20  # OFDM_LDPC_MAX_ITER: iterations the decode chain gives a code word
FCS_OVERHEAD = 8  # OFDM_FCS_OVERHEAD: the envelope's length word and check word
CONV_RATE_1_2, CONV_RATE_2_3, CONV_RATE_3_4 = 0, 1, 2
SOFT_LLR_SCALE = 32.0  # OFDM_SOFT_LLR_SCALE (include/ofdm_hip.h): the llr_scale of the soft decode chain
CFO_OFF, CFO_SIGNED, CFO_ABS = 0, 1, 2
# EXT-8 (tests/cfo_wide_ref.py is the definition): the Schmidl-Cox phase alone acquires +-pi / S rad/sample, +-0.4 sub-carrier spacings;
# CFO_WIDE resolves the whole multiples of 2 pi / S from the training blocks: +-6.8 spacings with the chain's span of 8
CFO_WIDE = 3
CFO_WIDE_SPAN = 8       # OFDM_CFO_WIDE_SPAN: hypotheses m in [-8, 8] in the decode chains
CFO_WIDE_MAX_SPAN = 32  # OFDM_CFO_WIDE_MAX_SPAN: the largest span Context.cfo_wide takes
FRAME_OK, FRAME_SHORT, FRAME_NOSYNC, FRAME_BADTIMING, FRAME_HEADER = 0, -1, -2, -3, -4
FRAME_UNCORRECTABLE = -5  # ECC_RS255*: an outer RS block with more than 16 byte errors (the reference returns None); ECC_LDPC648: a code word did not converge
FRAME_FCS = -6  # ECC_FCS + mode: the delivered row is not a valid envelope (length word or CRC-32 wrong)
SYNC_SCHMIDL_COX, SYNC_REFERENCE = 0, 1
RX_AUTO, RX_STAGED = 0, 1
# channel estimate of the receive chain: the reference's bin-by-bin one, or that one denoised by a weighted least-squares fit of cp_len
# taps (EXT-5; tests/chest_ref.py is the definition)
# Under SYNC_SCHMIDL_COX ofdm_create refuses CHEST_WLS (and CFO_WIDE) with sync_backoff >= 3 cp_len / 4: the tap window ends there
CHEST_LS, CHEST_WLS = 0, 1
# ofdm_rx_quality_batch: indices into a frame's row of QUALITY_FIELDS floats (EXT-6; tests/quality_ref.py is the definition)
Q_VALID, Q_NOISE_VAR, Q_GAIN, Q_SNR, Q_LLR_UNIT, Q_EVM2, Q_POINTS = 0, 1, 2, 3, 4, 5, 6
QUALITY_FIELDS = 8
# EXT-11 (tests/noise_weight_ref.py is the definition): what the decode chains weigh their LLRs by -- the channel weight alone, or that
# times q_k = min(1, mean noise / noise of carrier k), measured per frame from the scatter of the five training blocks
LLRW_CHANNEL, LLRW_NOISE = 0, 1
# EXT-9: sc16 = interleaved little-endian int16 I/Q (UHD's wire format), int16 arrays / tensors of shape [..., 2]; x = int16 * scale as ONE
# rounded f32 product (tests/sc16_ref.py is the definition)
SC16_DEFAULT_SCALE = 1.0 / 32768.0  # OFDM_SC16_DEFAULT_SCALE
DEFAULT_TUNING: dict = {}  # merged under every Context's `tuning=` (tools/tune_env.py fills it; empty in tests, bench and smoke)


class OfdmError(RuntimeError):
    pass


class DecodeError(OfdmError):
    """`Err(anyhow!(..))` of decode (src/receiver.rs:27-29)."""


def _check(lib, rc: int, what: str, ctx=None):
    if rc != 0:
        extra = f" (hipError {lib.ofdm_last_hip_error(ctx)})" if ctx is not None and rc == -4 else ""
        raise OfdmError(f"{what}: {lib.ofdm_strerror(rc).decode()}{extra}")


def default_pilots(n_fft: int = 64):
    """(preamble[n_fft+cp], training[n_fft]) complex128 -- SplitMix64 stand-ins for the StdRng tables of
    src/transmitter.rs:75-96 (same seeds 100 / 50, same draw order and scaling)."""
    lib = _lib.load()
    cp = n_fft // 4
    pre = np.zeros(n_fft + cp, np.complex128)
    trn = np.zeros(n_fft, np.complex128)
    _check(lib, lib.ofdm_default_pilots(n_fft, cp, pre.ctypes.data, trn.ctypes.data), "ofdm_default_pilots")
    return pre, trn


def stdrng_pilots(n_fft: int = 64):
    """(preamble[n_fft+cp], training[n_fft]) as the reference draws them: rand 0.8 StdRng (ChaCha12), seeds 100 / 50
    (src/transmitter.rs:75-96).  Restated from the published algorithm; unverified against a running `rand`."""
    lib = _lib.load()
    cp = n_fft // 4
    pre = np.zeros(n_fft + cp, np.complex128)
    trn = np.zeros(n_fft, np.complex128)
    _check(lib, lib.ofdm_stdrng_pilots(n_fft, cp, pre.ctypes.data, trn.ctypes.data), "ofdm_stdrng_pilots")
    return pre, trn


def create_transmission_bytes(data: bytes) -> bytes:
    """utils::create_transmission_bytes (src/utils.rs:97-136): outer RS(255,223) blocks, host side."""
    lib = _lib.load()
    src = np.frombuffer(bytes(data), np.uint8).copy()
    out = np.zeros(lib.ofdm_rs255_encoded_len(src.size), np.uint8)
    _check(lib, lib.ofdm_rs255_encode(src.ctypes.data if src.size else None, src.size, out.ctypes.data), "ofdm_rs255_encode")
    return bytes(out)


def decipher_transmission_bytes(code: bytes) -> Optional[bytes]:
    """utils::decipher_transmission_bytes (src/utils.rs:150-180): None where the reference returns None
    (a block with more than 16 byte errors)."""
    lib = _lib.load()
    src = np.frombuffer(bytes(code), np.uint8).copy()
    out = np.zeros(lib.ofdm_rs255_decoded_len(src.size), np.uint8)
    rc = lib.ofdm_rs255_decode(src.ctypes.data if src.size else None, src.size, out.ctypes.data, None)
    if rc == -6:
        return None
    _check(lib, rc, "ofdm_rs255_decode")
    return bytes(out)


def crc32(data: bytes) -> int:
    """ofdm_crc32: the CRC-32 of IEEE 802.3 / zlib, as the library's host code computes it (no GPU needed)."""
    lib = _lib.load()
    src = np.frombuffer(bytes(data), np.uint8).copy()
    return int(lib.ofdm_crc32(src.ctypes.data if src.size else None, src.size))  # (no bytes: NULL, 0 -> 0 = crc32(b""))


def sig_to_bytes(sig) -> bytes:
    """utils::sig_to_bytes (src/utils.rs:228-236): Complex64 samples -> native-endian f32 (re, im) pairs, the `fc32` format of
    UHD's `--type float` tools (data/transmit.sh:1) and the layout every kernel of this library reads and writes."""
    return np.ascontiguousarray(np.asarray(sig), dtype=np.complex64).tobytes()


def bytes_to_sig(buf: bytes) -> np.ndarray:
    """utils::bytes_to_sig (src/utils.rs:238-254): fc32 bytes -> Complex64 samples (a trailing partial sample is dropped, as
    `as_chunks` drops it)."""
    n = len(buf) // 8
    return np.frombuffer(buf, dtype=np.complex64, count=n).astype(np.complex128)


def locking_signal(length: int = 80) -> np.ndarray:
    """src/transmitter.rs:60-72 (host-side constant; the library builds the same table into its frame header)."""
    v = 0.5 * (np.arange(length) / (2.0 * length) + 0.5)
    return np.fft.fftshift(v).astype(np.complex128) if length % 2 == 0 else np.roll(v, -((length + 1) // 2)) + 0j


def preamble(length: int = 80) -> np.ndarray:
    return default_pilots(length * 4 // 5)[0]


def training_signals(length: int = 64) -> np.ndarray:
    return default_pilots(length)[1]


def pinned_empty(shape, dtype) -> np.ndarray:
    """A numpy array in page-locked host memory (ofdm_host_alloc): what the host-buffer entry points DMA in place.  The memory
    is returned to the driver when the array (and every view of it) is gone."""
    import weakref

    lib = _lib.load()
    dt = np.dtype(dtype)
    n = int(np.prod(shape)) * dt.itemsize
    ptr = C.c_void_p()
    _check(lib, lib.ofdm_host_alloc(max(n, 1), C.byref(ptr)), "ofdm_host_alloc")
    buf = (C.c_char * max(n, 1)).from_address(ptr.value)
    arr = np.frombuffer(buf, dtype=np.uint8, count=n).view(dt).reshape(shape)
    weakref.finalize(buf, lib.ofdm_host_free, C.c_void_p(ptr.value))
    return arr


def _sc16_host(a, what: str) -> np.ndarray:
    a = np.asarray(a)
    if a.dtype != np.int16 or a.ndim < 1 or a.shape[-1] != 2:
        raise OfdmError(f"{what}: expected an int16 array of shape [..., 2]")
    return np.ascontiguousarray(a)


def sc16_widen(samples, scale: float = SC16_DEFAULT_SCALE) -> np.ndarray:
    """ofdm_sc16_widen on the host (no device): int16 [..., 2] -> complex64 [...], x = int16 * scale per component."""
    a = _sc16_host(samples, "sc16_widen")
    out = np.empty(a.shape[:-1], np.complex64)
    lib = _lib.load()
    _check(lib, lib.ofdm_sc16_widen(_host(a), out.size, scale, _host(out)), "ofdm_sc16_widen")
    return out


def sc16_narrow(samples, scale: float = 1.0 / SC16_DEFAULT_SCALE):
    """ofdm_sc16_narrow on the host (no device): complex64 [...] -> (int16 [..., 2], clipped components); q = clamp(rint(x * scale))."""
    x = np.ascontiguousarray(samples, dtype=np.complex64)
    out = np.empty(x.shape + (2,), np.int16)
    clipped = C.c_int64()
    lib = _lib.load()
    _check(lib, lib.ofdm_sc16_narrow(_host(x), x.size, scale, _host(out), C.byref(clipped)), "ofdm_sc16_narrow")
    return out, int(clipped.value)


def dc_block_default(n_fft: int = 64) -> int:
    """ofdm_dc_block_default (EXT-15): the default window of the DC blocker in blocks of 64 samples, ceil(3 S / 64)."""
    lib = _lib.load()
    m = int(lib.ofdm_dc_block_default(int(n_fft), int(n_fft) // 4))
    _check(lib, min(m, 0), "ofdm_dc_block_default")
    return m


def dc_block_host(samples, blocks: int, scale: Optional[float] = None) -> np.ndarray:
    """ofdm_dc_block / ofdm_dc_block_sc16 (EXT-15): the definition of the DC blocker on one whole stream, on the host, no GPU: complex64
    [n] in, complex64 [n] out.  An int16 array of shape [n, 2] takes scale= and is widened by ofdm_sc16_widen's rule first."""
    lib = _lib.load()
    if np.asarray(samples).dtype == np.int16:
        if scale is None:
            raise OfdmError("dc_block_host: int16 samples need scale=")
        a = _sc16_host(samples, "dc_block_host").reshape(-1, 2)
        out = np.empty(a.shape[0], np.complex64)
        _check(lib, lib.ofdm_dc_block_sc16(_host(a), a.shape[0], float(scale), int(blocks), _host(out)), "ofdm_dc_block_sc16")
        return out
    x = np.ascontiguousarray(samples, dtype=np.complex64).reshape(-1)
    out = np.empty(x.size, np.complex64)
    _check(lib, lib.ofdm_dc_block(_host(x), x.size, int(blocks), _host(out)), "ofdm_dc_block")
    return out


DDC_TAPS_PER_PHASE = 24
DDC_PHASE_MOD = 1 << 20


def ddc_rotor_tables():
    """ofdm_ddc_rotor_tables (EXT-16): the coarse and the fine rotor table, complex64 [1024] each -- the bytes the host definition uses
    and the device is given"""
    lib = _lib.load()
    c, f = np.empty(1024, np.complex64), np.empty(1024, np.complex64)
    _check(lib, lib.ofdm_ddc_rotor_tables(_host(c), _host(f)), "ofdm_ddc_rotor_tables")
    return c, f


def ddc_out_len(n: int, decim: int, n_taps: int) -> int:
    """ofdm_ddc_out_len (EXT-16): M(n), the outputs n input samples give: 0 for n < n_taps, else (n - n_taps) // decim + 1"""
    lib = _lib.load()
    m = int(lib.ofdm_ddc_out_len(int(n), int(decim), int(n_taps)))
    _check(lib, min(m, 0), "ofdm_ddc_out_len")
    return m


def ddc_inc_for(f0: float) -> int:
    """ofdm_ddc_inc_for (EXT-16): the phase increment that brings f0 (cycles per input sample, |f0| <= 0.5) to 0"""
    lib = _lib.load()
    inc = C.c_int32()
    _check(lib, lib.ofdm_ddc_inc_for(float(f0), C.byref(inc)), "ofdm_ddc_inc_for")
    return int(inc.value)


def ddc_design(decim: int, taps_per_phase: int = DDC_TAPS_PER_PHASE) -> np.ndarray:
    """ofdm_ddc_design (EXT-16): the Hamming-windowed sinc of taps_per_phase * decim taps with the cutoff 0.5 / decim, float32"""
    lib = _lib.load()
    if not (1 <= int(decim) <= 64 and 1 <= int(taps_per_phase) <= 64):
        raise OfdmError("ddc_design: decim and taps_per_phase are 1 .. 64")
    taps = np.empty(int(decim) * int(taps_per_phase), np.float32)
    _check(lib, lib.ofdm_ddc_design(int(decim), int(taps_per_phase), _host(taps)), "ofdm_ddc_design")
    return taps


def _ddc_taps(decim: int, taps) -> np.ndarray:
    return ddc_design(decim) if taps is None else np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)


def ddc_host(samples, decim: int, phase_inc: int = 0, taps=None, scale: Optional[float] = None) -> np.ndarray:
    """ofdm_ddc / ofdm_ddc_sc16 (EXT-16): the definition of the down-converter on one whole stream, on the host, no GPU: complex64 [n]
    in, complex64 [M(n)] out.  taps None: ddc_design(decim).  An int16 array of shape [n, 2] takes scale= and is widened by
    ofdm_sc16_widen's rule first."""
    lib = _lib.load()
    h = _ddc_taps(decim, taps)
    n_out = C.c_int64()
    inc = int(phase_inc) % DDC_PHASE_MOD
    if np.asarray(samples).dtype == np.int16:
        if scale is None:
            raise OfdmError("ddc_host: int16 samples need scale=")
        a = _sc16_host(samples, "ddc_host").reshape(-1, 2)
        out = np.empty(max(a.shape[0] // max(int(decim), 1) + 1, 1), np.complex64)
        _check(lib, lib.ofdm_ddc_sc16(_host(a), a.shape[0], float(scale), int(decim), inc, _host(h), h.size, _host(out), out.size,
                                      C.byref(n_out)), "ofdm_ddc_sc16")
        return out[: int(n_out.value)].copy()
    x = np.ascontiguousarray(samples, dtype=np.complex64).reshape(-1)
    out = np.empty(max(x.size // max(int(decim), 1) + 1, 1), np.complex64)
    _check(lib, lib.ofdm_ddc(_host(x), x.size, int(decim), inc, _host(h), h.size, _host(out), out.size, C.byref(n_out)), "ofdm_ddc")
    return out[: int(n_out.value)].copy()


def _host(a: Optional[np.ndarray]):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _dev(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def conv_max_steps(bits: int, rate: int) -> int:
    """The largest T with ofdm_conv_k7_kept_bits(T, rate) <= bits (the library's conv_max_steps; tests/framed_ref.max_steps)."""
    return (bits // 2, 2 * (bits // 3) + (bits % 3 == 2), 3 * (bits // 4) + (0, 0, 1, 2)[bits % 4])[rate]


class Context:
    """One (GPU, stream) context = `ofdm_ctx`.  Tensors passed in must live on this context's device."""

    def __init__(self, n_fft: int = 64, modulation: int = BPSK, guard_bands: bool = False, ecc: int = ECC_NONE,
                 device: int = 0, preamble: Optional[np.ndarray] = None, training: Optional[np.ndarray] = None,
                 sync_window_reps: int = 3, sync_backoff: int = 4, cfo_mode: int = CFO_SIGNED,
                 sync_threshold: float = 0.5, use_torch_stream: bool = True, pilots: str = "default",
                 sync_mode: int = SYNC_SCHMIDL_COX, rx_path: int = RX_AUTO, tuning: Optional[dict] = None,
                 chest_mode: int = CHEST_LS, llr_weight: int = LLRW_CHANNEL):
        self.lib = _lib.load()
        if pilots == "stdrng":  # the reference's own tables (restated, unverified) unless explicit tables are given
            sp, st = stdrng_pilots(n_fft)
            preamble = sp if preamble is None else preamble
            training = st if training is None else training
        elif pilots != "default":
            raise OfdmError("pilots must be 'default' or 'stdrng'")
        if not torch.cuda.is_available():
            raise OfdmError("no GPU visible: the OFDM hot path has no CPU fallback")
        self.device = torch.device("cuda", device)
        p = _lib.Params()
        _check(self.lib, self.lib.ofdm_default_params(C.byref(p)), "ofdm_default_params")
        p.n_fft, p.cp_len, p.modulation, p.guard_bands, p.ecc = n_fft, n_fft // 4, modulation, int(guard_bands), ecc
        p.sync_window_reps, p.sync_backoff, p.cfo_mode, p.sync_threshold = (sync_window_reps, sync_backoff, cfo_mode,
                                                                            sync_threshold)
        p.sync_mode = sync_mode
        p.rx_path = rx_path
        p.chest_mode = chest_mode
        self.params = p
        pre = None if preamble is None else np.ascontiguousarray(preamble, dtype=np.complex128)
        trn = None if training is None else np.ascontiguousarray(training, dtype=np.complex128)
        if pre is not None and pre.size != n_fft + n_fft // 4:
            raise OfdmError("preamble must hold n_fft + cp samples")
        if trn is not None and trn.size != n_fft:
            raise OfdmError("training must hold n_fft bins")
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream if use_torch_stream else 0
        h = C.c_void_p()
        rc = self.lib.ofdm_create(C.byref(p), None if pre is None else pre.ctypes.data,
                                  None if trn is None else trn.ctypes.data, device, C.c_void_p(stream), C.byref(h))
        _check(self.lib, rc, "ofdm_create")
        self.h = h
        self.n_fft, self.cp, self.S = n_fft, n_fft // 4, n_fft + n_fft // 4
        self.modulation, self.guard_bands, self.ecc = modulation, bool(guard_bands), ecc
        self.data_carriers = self.lib.ofdm_data_carriers(h)
        self.bytes_per_symbol = self.lib.ofdm_bytes_per_symbol(h)
        for k, v in {**DEFAULT_TUNING, **(tuning or {})}.items():
            self.set_tuning(k, v)
        if float(np.float32(sync_threshold)) != float(sync_threshold):
            # ofdm_params carries the threshold as a float; a double that a float cannot hold goes through the laboratory key
            self.set_tuning("sync_threshold_bits", int(np.float64(sync_threshold).view(np.int64)))
        if llr_weight != LLRW_CHANNEL:
            self.set_llr_weight(llr_weight)

    def close(self):
        if getattr(self, "h", None):
            for s in list(getattr(self, "_streams", ())):  # a stream is destroyed before its context (include/ofdm_hip.h)
                s.close()
            self.lib.ofdm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------------------------- helpers
    def _ck(self, rc, what):
        _check(self.lib, rc, what, self.h)

    def synchronize(self):
        self._ck(self.lib.ofdm_synchronize(self.h), "ofdm_synchronize")

    def set_tuning(self, key: str, value: int):
        """ofdm_set_tuning: per-context A/B switches and grid shapes (keys in include/ofdm_hip.h)."""
        self._ck(self.lib.ofdm_set_tuning(self.h, key.encode(), int(value)), f"ofdm_set_tuning({key})")

    def get_tuning(self, key: str) -> int:
        v = C.c_int64()
        self._ck(self.lib.ofdm_get_tuning(self.h, key.encode(), C.byref(v)), f"ofdm_get_tuning({key})")
        return int(v.value)

    def set_llr_weight(self, mode: int):
        """ofdm_set_llr_weight: LLRW_CHANNEL (the default) or LLRW_NOISE -- under it every decode entry point that forms LLRs multiplies
        them by the per-carrier noise weight of noise_bins (EXT-11)."""
        self._ck(self.lib.ofdm_set_llr_weight(self.h, int(mode)), "ofdm_set_llr_weight")

    def get_llr_weight(self) -> int:
        v = C.c_int32()
        self._ck(self.lib.ofdm_get_llr_weight(self.h, C.byref(v)), "ofdm_get_llr_weight")
        return int(v.value)

    def last_dispatch(self) -> str:
        """The kernels the last entry point launched, e.g. 'k_rx_prepare+k_rxframe64<finish>' (ofdm_last_dispatch)."""
        buf = C.create_string_buffer(512)
        n = self.lib.ofdm_last_dispatch(self.h, buf, len(buf))
        if n < 0:
            self._ck(n, "ofdm_last_dispatch")
        return buf.value.decode()

    def coded_len(self, payload_bytes: int) -> int:
        return int(self.lib.ofdm_coded_len(self.h, payload_bytes))

    def data_symbols(self, payload_bytes: int) -> int:
        return int(self.lib.ofdm_data_symbols(self.h, payload_bytes))

    def frame_samples(self, payload_bytes: int) -> int:
        return int(self.lib.ofdm_frame_samples(self.h, payload_bytes))

    def to_device(self, a, dtype=None) -> torch.Tensor:
        if isinstance(a, torch.Tensor):
            t = a.to(self.device)
            return t if dtype is None else t.to(dtype)
        arr = np.ascontiguousarray(a)
        if np.iscomplexobj(arr):
            arr = arr.astype(np.complex64)  # sig_to_bytes: f64 -> f32 pairs (src/utils.rs:228-236)
        t = torch.from_numpy(arr).to(self.device)
        return t if dtype is None else t.to(dtype)

    def _cx(self, t: torch.Tensor) -> torch.Tensor:
        if t.dtype != torch.complex64 or not t.is_contiguous() or t.device != self.device:
            raise OfdmError("expected a contiguous complex64 tensor on the context's device")
        return t

    def _u8(self, t: torch.Tensor) -> torch.Tensor:
        if t.dtype != torch.uint8 or not t.is_contiguous() or t.device != self.device:
            raise OfdmError("expected a contiguous uint8 tensor on the context's device")
        return t

    def empty(self, shape, dtype) -> torch.Tensor:
        return torch.empty(shape, dtype=dtype, device=self.device)

    def _sc16(self, t: torch.Tensor) -> torch.Tensor:
        """[n_frames, stride, 2] (or [stride, 2]) int16 on the device; rows may be views with a stride of their own (a row start at
        any sample), the samples of a row are contiguous."""
        if t.dtype != torch.int16 or t.device != self.device or t.dim() < 2 or t.shape[-1] != 2 or t.stride(-1) != 1 or \
                (t.shape[-2] > 1 and t.stride(-2) != 2):
            raise OfdmError("expected an int16 tensor of shape [..., 2] on the context's device, samples of a row contiguous")
        if t.dim() == 2:
            t = t.unsqueeze(0)
        if t.dim() != 3 or (t.shape[0] > 1 and t.stride(0) % 2):
            raise OfdmError("expected int16 rows [n_frames, samples, 2] a whole number of samples apart")
        return t

    @staticmethod
    def _rows(t: torch.Tensor):
        """(n_frames, samples per row, row stride in samples) of a _sc16 tensor"""
        n, ln = t.shape[0], t.shape[1]
        return n, ln, (t.stride(0) // 2 if n > 1 else ln)

    # ---------------------------------------------------------------- stage level
    def fft(self, x: torch.Tensor, inverse: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """SignalMut::fft / ifft (src/signals/mod.rs:27-58) over the last dim (== n_fft)."""
        x = self._cx(x)
        assert x.shape[-1] == self.n_fft
        out = torch.empty_like(x) if out is None else self._cx(out)
        self._ck(self.lib.ofdm_fft_batch(self.h, _dev(x), _dev(out), x.numel() // self.n_fft, int(inverse)), "fft")
        return out

    def prefix_block(self, freq: torch.Tensor) -> torch.Tensor:
        """prefix_block::<N, N/4> (src/transmitter.rs:168-181): [..., N] bins -> [..., N+CP] samples."""
        freq = self._cx(freq)
        assert freq.shape[-1] == self.n_fft
        out = self.empty(freq.shape[:-1] + (self.S,), torch.complex64)
        self._ck(self.lib.ofdm_ifft_cp_batch(self.h, _dev(freq), _dev(out), freq.numel() // self.n_fft), "ifft_cp")
        return out

    def tx_symbols(self, data: torch.Tensor, n_sym: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """modulate + encode_block + prefix_block fused (src/transmitter.rs:40-53): a continuous byte stream ->
        [n_sym, n_fft + cp] samples, identical to the three staged calls."""
        data = self._u8(data).reshape(-1)
        nb = data.numel()
        need = (nb + self.bytes_per_symbol - 1) // self.bytes_per_symbol
        n_sym = need if n_sym is None else n_sym
        out = self.empty((n_sym, self.S), torch.complex64) if out is None else self._cx(out)
        assert out.numel() == n_sym * self.S
        self._ck(self.lib.ofdm_tx_symbols_batch(self.h, _dev(data), nb, _dev(out), n_sym), "tx_symbols")
        return out

    def unprefix_block(self, blocks: torch.Tensor) -> torch.Tensor:
        """unprefix_block (src/receiver.rs:99-104): [..., N+CP] samples -> [..., N] bins."""
        blocks = self._cx(blocks)
        assert blocks.shape[-1] == self.S
        out = self.empty(blocks.shape[:-1] + (self.n_fft,), torch.complex64)
        self._ck(self.lib.ofdm_unprefix_batch(self.h, _dev(blocks), _dev(out), blocks.numel() // self.S), "unprefix")
        return out

    def modulate(self, data: torch.Tensor) -> torch.Tensor:
        """modulate (src/transmitter.rs:108-140): uint8[n] -> complex64[ceil(8n/bps)]."""
        data = self._u8(data)
        n = (data.numel() * 8 + self.modulation - 1) // self.modulation
        out = self.empty((n,), torch.complex64)
        self._ck(self.lib.ofdm_qam_map_batch(self.h, _dev(data), data.numel(), _dev(out)), "qam_map")
        return out

    def demodulate(self, sym: torch.Tensor, want_indices: bool = False):
        """demodulate (src/receiver.rs:147-190): complex64[n], n % 8 == 0 -> uint8[n*bps/8]."""
        sym = self._cx(sym)
        n = sym.numel()
        if n % 8 != 0:
            raise OfdmError("demodulate: symbol count must be a multiple of 8 (receiver.rs:153)")
        out = self.empty((n * self.modulation // 8,), torch.uint8)
        idx = self.empty((n,), torch.uint8) if want_indices else None
        self._ck(self.lib.ofdm_qam_demap_batch(self.h, _dev(sym), n, _dev(out), _dev(idx)), "qam_demap")
        return (out, idx) if want_indices else out

    def encode_block(self, data: torch.Tensor) -> torch.Tensor:
        """encode_block (src/transmitter.rs:144-165): [n_sym, data_carriers] -> [n_sym, N]."""
        data = self._cx(data)
        assert data.shape[-1] == self.data_carriers
        out = self.empty(data.shape[:-1] + (self.n_fft,), torch.complex64)
        self._ck(self.lib.ofdm_encode_block_batch(self.h, _dev(data), _dev(out), data.numel() // self.data_carriers),
                 "encode_block")
        return out

    def normalize(self, frames: torch.Tensor) -> torch.Tensor:
        """normalize (src/transmitter.rs:183-194), in place, per row."""
        frames = self._cx(frames)
        f2 = frames.view(-1, frames.shape[-1])
        self._ck(self.lib.ofdm_normalize_batch(self.h, _dev(f2), f2.shape[0], f2.shape[1], f2.shape[1]), "normalize")
        return frames

    def hamming74_encode(self, data: torch.Tensor) -> torch.Tensor:
        data = self._u8(data)
        out = self.empty(((data.numel() + 3) // 4 * 7,), torch.uint8)
        self._ck(self.lib.ofdm_hamming74_encode(self.h, _dev(data), data.numel(), _dev(out)), "hamming74_encode")
        return out

    def hamming74_decode(self, code: torch.Tensor):
        code = self._u8(code)
        out = self.empty((code.numel() // 7 * 4,), torch.uint8)
        fixed = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._ck(self.lib.ofdm_hamming74_decode(self.h, _dev(code), code.numel(), _dev(out), _dev(fixed)),
                 "hamming74_decode")
        return out, fixed

    def hamming74_decode_soft(self, llr: torch.Tensor) -> torch.Tensor:
        """ofdm_hamming74_decode_soft: int8 LLRs (positive = bit 1), floor(n / 56) blocks of 8 codewords -> 4 bytes per block (ML)."""
        if llr.dtype != torch.int8 or not llr.is_contiguous() or llr.device != self.device:
            raise OfdmError("expected a contiguous int8 tensor on the context's device")
        out = self.empty((llr.numel() // 56 * 4,), torch.uint8)
        self._ck(self.lib.ofdm_hamming74_decode_soft(self.h, _dev(llr), llr.numel(), _dev(out)), "hamming74_decode_soft")
        return out

    def conv_encode(self, data: torch.Tensor, rate: Optional[int] = None) -> torch.Tensor:
        """ofdm_conv_k7_encode: rows of data [n_frames, n_bytes] (uint8; the rows may be strided) -> [n_frames, 2 (n_bytes + 1)] coded
        bytes of the K = 7 rate-1/2 code (133 / 171 octal), one zero tail byte appended to every row.
        rate (CONV_RATE_*): ofdm_conv_k7_encode_punctured -> [n_frames, ceil(kept(8 (n_bytes + 1), rate) / 8)]."""
        if data.dtype != torch.uint8 or data.dim() != 2 or data.device != self.device or (data.shape[1] > 1 and data.stride(1) != 1):
            raise OfdmError("expected a uint8 tensor [n_frames, n_bytes] with contiguous rows on the context's device")
        n, nb = data.shape
        stride = data.stride(0) if n > 1 else nb
        if rate is not None:
            kept = int(self.lib.ofdm_conv_k7_kept_bits(8 * (nb + 1), int(rate)))
            self._ck(min(kept, 0), "conv_k7_kept_bits")
            out = self.empty((n, (kept + 7) // 8), torch.uint8)
            self._ck(self.lib.ofdm_conv_k7_encode_punctured(self.h, _dev(data), n, stride, nb, int(rate), _dev(out), out.shape[1]),
                     "conv_k7_encode_punctured")
            return out
        out = self.empty((n, 2 * (nb + 1)), torch.uint8)
        self._ck(self.lib.ofdm_conv_k7_encode(self.h, _dev(data), n, stride, nb, _dev(out), out.shape[1]), "conv_k7_encode")
        return out

    def viterbi_decode_soft(self, llr: torch.Tensor, n_steps: Optional[int] = None, terminated: bool = True,
                            rate: Optional[int] = None) -> torch.Tensor:
        """ofdm_conv_k7_decode_soft: rows of llr [n_frames, >= 2 n_steps] (int8, positive = bit 1; the rows may be strided) ->
        [n_frames, n_steps // 8] bytes, the exact Viterbi (maximum-likelihood) decode; n_steps defaults to the row length // 2.
        terminated: the traceback starts at state 0, otherwise at the best final state.
        rate (CONV_RATE_*): ofdm_conv_k7_decode_punctured, rows of the kept(n_steps, rate) LLRs of a punctured stream; n_steps is
        required then."""
        if llr.dtype != torch.int8 or llr.dim() != 2 or llr.device != self.device or (llr.shape[1] > 1 and llr.stride(1) != 1):
            raise OfdmError("expected an int8 tensor [n_frames, >= 2 n_steps] with contiguous rows on the context's device")
        n, width = llr.shape
        if rate is not None:
            if n_steps is None or n_steps < 0:
                raise OfdmError("viterbi_decode_soft: a punctured row does not tell its n_steps")
            kept = int(self.lib.ofdm_conv_k7_kept_bits(int(n_steps), int(rate)))
            self._ck(min(kept, 0), "conv_k7_kept_bits")
            if kept > width:
                raise OfdmError("viterbi_decode_soft: rows must hold kept(n_steps, rate) LLRs")
            out = self.empty((n, int(n_steps) // 8), torch.uint8)
            self._ck(self.lib.ofdm_conv_k7_decode_punctured(self.h, _dev(llr), n, llr.stride(0) if n > 1 else width, int(n_steps), int(rate),
                                                            int(bool(terminated)), _dev(out), out.shape[1]), "conv_k7_decode_punctured")
            return out
        n_steps = width // 2 if n_steps is None else int(n_steps)
        if n_steps < 0 or 2 * n_steps > width:
            raise OfdmError("viterbi_decode_soft: rows must hold 2 * n_steps LLRs")
        out = self.empty((n, n_steps // 8), torch.uint8)
        stride = llr.stride(0) if n > 1 else width
        self._ck(self.lib.ofdm_conv_k7_decode_soft(self.h, _dev(llr), n, stride, n_steps, int(bool(terminated)), _dev(out), out.shape[1]),
                 "conv_k7_decode_soft")
        return out

    def _rows_u8(self, t: torch.Tensor, what: str):
        if t.dtype != torch.uint8 or t.dim() != 2 or t.device != self.device or (t.shape[1] > 1 and t.stride(1) != 1):
            raise OfdmError(f"{what}: expected a uint8 tensor [n_frames, n_bytes] with contiguous rows on the context's device")
        n, nb = t.shape
        return n, nb, (t.stride(0) if n > 1 else nb)

    def _lens_i32(self, lens, n: int, what: str):
        if lens is None:
            return None
        lens = lens.to(device=self.device, dtype=torch.int32).contiguous()
        if lens.numel() != n:
            raise OfdmError(f"{what}: lens must hold one length per row")
        return lens

    def rs255_encode(self, data: torch.Tensor, lens: Optional[torch.Tensor] = None) -> torch.Tensor:
        """ofdm_rs255_encode_batch: rows of data [n_frames, n_bytes] (uint8; the rows may be strided) -> [n_frames, 255 (n_bytes // 223 + 1)]
        RS(255,223) code bytes, every row what create_transmission_bytes makes of it.  lens (int32 [n_frames], optional): the rows' own
        lengths (clamped to [0, n_bytes]); a row is zero behind its own 255 (len // 223 + 1) bytes."""
        n, nb, stride = self._rows_u8(data, "rs255_encode")
        lens = self._lens_i32(lens, n, "rs255_encode")
        out = self.empty((n, int(self.lib.ofdm_rs255_encoded_len(nb))), torch.uint8)
        self._ck(self.lib.ofdm_rs255_encode_batch(self.h, _dev(data), n, stride, _dev(lens), nb, _dev(out), out.shape[1]), "rs255_encode_batch")
        return out

    def rs255_decode(self, code: torch.Tensor, lens: Optional[torch.Tensor] = None):
        """ofdm_rs255_decode_batch: rows of code [n_frames, n_code] (uint8; the rows may be strided) -> (bytes [n_frames, 223 (n_code // 255 + 1)],
        out_len int32 [n_frames], corrected int32 [n_frames]), every row what decipher_transmission_bytes makes of its own len bytes.
        corrected = the row's corrected bytes, or -1 if a block has more than 16 byte errors: that block's data bytes are delivered as
        received, the other blocks corrected.  Bytes behind out_len are not written."""
        n, nc, stride = self._rows_u8(code, "rs255_decode")
        lens = self._lens_i32(lens, n, "rs255_decode")
        out = self.empty((n, int(self.lib.ofdm_rs255_decoded_len(nc))), torch.uint8)
        out_len, fixed = self.empty((n,), torch.int32), self.empty((n,), torch.int32)
        self._ck(self.lib.ofdm_rs255_decode_batch(self.h, _dev(code), n, stride, _dev(lens), nc, _dev(out), out.shape[1], _dev(out_len),
                                                  _dev(fixed)), "rs255_decode_batch")
        return out, out_len, fixed

    @staticmethod
    def _ldpc_k(rate: int, what: str) -> int:
        if rate not in (0, 1, 2, 3):
            raise OfdmError(f"{what}: rate must be 0 (1/2), 1 (2/3), 2 (3/4) or 3 (5/6)")
        return LDPC_INFO_BYTES[rate]

    def ldpc_encode(self, info: torch.Tensor, rate: int = 0) -> torch.Tensor:
        """ofdm_ldpc648_encode_batch / _encode_rate_batch: rows of info [n_frames, K n_cw] (uint8; the rows may be strided; K = 40 / 53 /
        60 / 67 for rate 0 .. 3) -> [n_frames, 80 n_cw] code bytes, every K-byte block coded on its own (the info bytes, then 80 - K
        parity bytes)."""
        k = self._ldpc_k(rate, "ldpc_encode")
        n, nb, stride = self._rows_u8(info, "ldpc_encode")
        if nb % k:
            raise OfdmError(f"ldpc_encode: rows must hold whole {k}-byte blocks")
        out = self.empty((n, 80 * (nb // k)), torch.uint8)
        if rate:
            self._ck(self.lib.ofdm_ldpc648_encode_rate_batch(self.h, _dev(info), n, max(stride, nb), nb // k, rate, _dev(out), out.shape[1]),
                     "ldpc648_encode_rate_batch")
            return out
        self._ck(self.lib.ofdm_ldpc648_encode_batch(self.h, _dev(info), n, max(stride, nb), nb // 40, _dev(out), 2 * nb), "ldpc648_encode_batch")
        return out

    def ldpc_decode(self, llr: torch.Tensor, max_iter: int = LDPC_MAX_ITER, rate: int = 0):
        """ofdm_ldpc648_decode_batch / _decode_rate_batch: rows of llr [n_frames, 640 n_cw] (int8, positive = bit 1; the rows may be
        strided) -> (bytes [n_frames, K n_cw], iters int32 [n_frames, n_cw]), K = 40 / 53 / 60 / 67 for rate 0 .. 3: layered normalised
        min-sum, every code word to convergence or max_iter (1 .. 64) iterations; iters = the iteration a code word converged at, 0 if
        it did not."""
        k = self._ldpc_k(rate, "ldpc_decode")
        if llr.dtype != torch.int8 or llr.dim() != 2 or llr.device != self.device or (llr.shape[1] > 1 and llr.stride(1) != 1):
            raise OfdmError("ldpc_decode: expected an int8 tensor [n_frames, 640 n_cw] with contiguous rows on the context's device")
        n, width = llr.shape
        if width % 640:
            raise OfdmError("ldpc_decode: rows must hold whole code words of 640 LLRs")
        n_cw = width // 640
        out, iters = self.empty((n, k * n_cw), torch.uint8), self.empty((n, n_cw), torch.int32)
        if rate:
            self._ck(self.lib.ofdm_ldpc648_decode_rate_batch(self.h, _dev(llr), n, max(llr.stride(0), width) if n > 1 else width, n_cw,
                                                             int(max_iter), rate, _dev(out), k * n_cw, _dev(iters)), "ldpc648_decode_rate_batch")
            return out, iters
        self._ck(self.lib.ofdm_ldpc648_decode_batch(self.h, _dev(llr), n, max(llr.stride(0), width) if n > 1 else width, n_cw, int(max_iter),
                                                    _dev(out), 40 * n_cw, _dev(iters)), "ldpc648_decode_batch")
        return out, iters

    def fcs_wrap(self, data: torch.Tensor, lens: Optional[torch.Tensor] = None, want_len: bool = False,
                 out: Optional[torch.Tensor] = None):
        """ofdm_fcs_wrap_batch: rows of data [n_frames, n_bytes] (uint8; the rows may be strided) -> [n_frames, n_bytes + 8] envelopes
        [u32 LE len][payload][u32 LE crc32 of both].  lens (int32 [n_frames], optional): the rows' own lengths (clamped to [0, n_bytes]);
        a row is zero behind its own len + 8 bytes.  want_len: also return the envelope lengths (int32 [n_frames]).  out (optional): a
        uint8 [n_frames, n_bytes + 8] tensor or view with contiguous rows."""
        n, nb, stride = self._rows_u8(data, "fcs_wrap")
        lens = self._lens_i32(lens, n, "fcs_wrap")
        if out is None:
            out = self.empty((n, nb + FCS_OVERHEAD), torch.uint8)
        on, onb, ostride = self._rows_u8(out, "fcs_wrap (out)")
        if on != n or onb != nb + FCS_OVERHEAD:
            raise OfdmError("fcs_wrap: out must hold n_frames rows of n_bytes + 8 bytes")
        out_len = self.empty((n,), torch.int32) if want_len else None
        self._ck(self.lib.ofdm_fcs_wrap_batch(self.h, _dev(data), n, stride, _dev(lens), nb, _dev(out), ostride, _dev(out_len)),
                 "fcs_wrap_batch")
        return (out, out_len) if want_len else out

    def fcs_check(self, rows: torch.Tensor, lens: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
        """ofdm_fcs_check_batch: rows [n_frames, n_row] (uint8; the rows may be strided), row f checked over its own lens[f] bytes
        (clamped to [0, n_row]; n_row without lens) -> (bytes [n_frames, max(n_row - 8, 0)], out_len int32 [n_frames], ok int32
        [n_frames]).  A valid row's payload is at the start of its output row with out_len = its length and ok = 1; an invalid row has
        out_len = 0 and ok = 0.  out (optional): a uint8 [n_frames, >= n_row - 8] tensor or view with contiguous rows."""
        n, nr, stride = self._rows_u8(rows, "fcs_check")
        lens = self._lens_i32(lens, n, "fcs_check")
        if out is None:
            out = self.empty((n, max(nr - FCS_OVERHEAD, 0)), torch.uint8)
        on, onb, ostride = self._rows_u8(out, "fcs_check (out)")
        if on != n or onb < nr - FCS_OVERHEAD:
            raise OfdmError("fcs_check: out must hold n_frames rows of at least n_row - 8 bytes")
        out_len, ok = self.empty((n,), torch.int32), self.empty((n,), torch.int32)
        self._ck(self.lib.ofdm_fcs_check_batch(self.h, _dev(rows), n, stride, _dev(lens), nr, _dev(out), max(ostride, onb), _dev(out_len), _dev(ok)),
                 "fcs_check_batch")
        return out, out_len, ok

    def decode_row_bytes(self, max_symbols: int) -> int:
        """Bytes per output row that the decode entry points are given for max_symbols (at least 4).  Modes without an outer code: the
        demodulated body, which bounds what each of them delivers.  ECC_RS255*: 223 (Lmax // 255 + 1), Lmax = the longest row the
        inner mode can deliver.  ECC_LDPC648*: the info bytes of the whole code words less the two length words.  ECC_FCS + mode: mode's
        row less the envelope's 8 bytes -- the rules of include/ofdm_hip.h."""
        body = max(max_symbols * self.bytes_per_symbol - 16, 0)
        fcs = self.ecc >= ECC_FCS
        ecc = self.ecc - ECC_FCS if fcs else self.ecc
        if ecc in (ECC_RS255, ECC_RS255_K7F_R12, ECC_RS255_K7F_R23, ECC_RS255_K7F_R34):
            lmax = body
            if ecc != ECC_RS255:  # a framed inner mode: the whole bytes of the steps a cut body still holds behind the length block
                lmax = conv_max_steps(8 * max(body - 18, 0), ecc - ECC_RS255_K7F_R12) // 8
            body = int(self.lib.ofdm_rs255_decoded_len(lmax))
        if ecc in (ECC_LDPC648, ECC_LDPC648_R23, ECC_LDPC648_R34, ECC_LDPC648_R56):
            body = max(LDPC_INFO_BYTES[0 if ecc == ECC_LDPC648 else ecc - ECC_LDPC648_R23 + 1] * (body // 80) - 8, 0)
        if fcs:
            body = max(body - FCS_OVERHEAD, 0)
        return max(body, 4)

    def sc_correlate(self, frames: torch.Tensor, frame_len: Optional[int] = None, n_lags: int = 0):
        """Schmidl-Cox timing / CFO per row of `frames` [n_frames, stride] -> (d_hat i32, f_delta f64, metric f32)."""
        frames = self._cx(frames)
        f2 = frames.view(-1, frames.shape[-1])
        n, stride = f2.shape
        frame_len = stride if frame_len is None else frame_len
        d = self.empty((n,), torch.int32)
        fd = self.empty((n,), torch.float64)
        m = self.empty((n,), torch.float32)
        self._ck(self.lib.ofdm_sc_correlate_batch(self.h, _dev(f2), n, stride, frame_len, n_lags, _dev(d), _dev(fd),
                                                  _dev(m)), "sc_correlate")
        return d, fd, m

    def xcorr(self, a: torch.Tensor, b: torch.Tensor, want_out: bool = False):
        """SignalRef::xcorr_fft (src/signals/mod.rs:186-217) per row of a [n, len] against b [nb]: (idx_max i32, peak f32
        [, the 2 len - 1 fft_shifted outputs])."""
        a = self._cx(a)
        a2 = a.view(-1, a.shape[-1])
        b = self._cx(b).reshape(-1)
        n, ln = a2.shape
        idx = self.empty((n,), torch.int32)
        pk = self.empty((n,), torch.float32)
        out = self.empty((n, 2 * ln - 1), torch.complex64) if want_out else None
        self._ck(self.lib.ofdm_xcorr_batch(self.h, _dev(a2), n, ln, ln, _dev(b), b.numel(), _dev(idx), _dev(pk), _dev(out),
                                           2 * ln - 1), "xcorr")
        return (idx, pk, out) if want_out else (idx, pk)

    def frequency_correction(self, left_right: torch.Tensor) -> torch.Tensor:
        """frequency_correction (src/receiver.rs:231-240): rows of [left(S) | right(S)] -> f64 |f_delta|."""
        x = self._cx(left_right)
        x2 = x.view(-1, 2 * self.S)
        out = self.empty((x2.shape[0],), torch.float64)
        self._ck(self.lib.ofdm_frequency_correction_batch(self.h, _dev(x2), x2.shape[0], 2 * self.S, self.S, _dev(out)),
                 "frequency_correction")
        return out

    def cfo_rotate(self, frames: torch.Tensor, f_delta: torch.Tensor, first_index: Optional[torch.Tensor] = None):
        """CFO derotation in place (src/receiver.rs:44-50)."""
        frames = self._cx(frames)
        f2 = frames.view(-1, frames.shape[-1])
        assert f_delta.dtype == torch.float64 and f_delta.numel() == f2.shape[0]
        self._ck(self.lib.ofdm_cfo_rotate_batch(self.h, _dev(f2), f2.shape[0], f2.shape[1], f2.shape[1], _dev(f_delta),
                                                _dev(first_index)), "cfo_rotate")
        return frames

    def estimate_channel(self, frames: torch.Tensor, offset: Optional[torch.Tensor] = None,
                         f_delta: Optional[torch.Tensor] = None, frame_len: Optional[int] = None) -> torch.Tensor:
        """estimate_channel (src/receiver.rs:212-229) on the training blocks 5..9 of each frame row."""
        frames = self._cx(frames)
        f2 = frames.view(-1, frames.shape[-1])
        hk = self.empty((f2.shape[0], self.n_fft), torch.complex64)
        self._ck(self.lib.ofdm_estimate_channel_batch(self.h, _dev(f2), f2.shape[0], f2.shape[1],
                                                      f2.shape[1] if frame_len is None else frame_len, _dev(offset),
                                                      _dev(f_delta), _dev(hk)), "estimate_channel")
        return hk

    def chest_smooth(self, hk: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """ofdm_chest_smooth_batch: rows of n_fft bins of a channel estimate -> the weighted least-squares fit of cp_len taps to every
        row, as n_fft bins again (EXT-5).  out may be hk itself.  Works whatever the context's chest_mode."""
        hk = self._cx(hk)
        assert hk.shape[-1] == self.n_fft
        out = torch.empty_like(hk) if out is None else self._cx(out)
        assert out.shape == hk.shape
        self._ck(self.lib.ofdm_chest_smooth_batch(self.h, _dev(hk), hk.numel() // self.n_fft, _dev(out)), "chest_smooth")
        return out

    def chest_window(self):
        """ofdm_chest_window: (first_tap, n_taps) = (-cp_len // 4, cp_len), the delays the denoised estimate may occupy."""
        first, n = C.c_int32(), C.c_int32()
        self._ck(self.lib.ofdm_chest_window(self.h, C.byref(first), C.byref(n)), "chest_window")
        return int(first.value), int(n.value)

    def rx_demod(self, frames: torch.Tensor, syms_per_frame: int, first_symbol: int = 0,
                 offset: Optional[torch.Tensor] = None, f_delta: Optional[torch.Tensor] = None,
                 hk: Optional[torch.Tensor] = None, frame_len: Optional[int] = None, want_soft: bool = False,
                 out: Optional[torch.Tensor] = None):
        """unprefix_block + equalise + decode_block + demodulate (src/receiver.rs:64-83) per OFDM symbol."""
        frames = self._cx(frames)
        f2 = frames.view(-1, frames.shape[-1])
        n, stride = f2.shape
        nb = syms_per_frame * self.bytes_per_symbol
        out = self.empty((n, nb), torch.uint8) if out is None else self._u8(out)
        soft = self.empty((n, syms_per_frame * self.data_carriers), torch.complex64) if want_soft else None
        hk_stride = 0
        if hk is not None:
            hk = self._cx(hk)
            hk_stride = self.n_fft if hk.dim() == 2 else 0  # [n_frames, N] per frame, [N] shared
            assert hk.shape[-1] == self.n_fft and (hk.dim() == 1 or hk.shape[0] == n)
        self._ck(self.lib.ofdm_rx_demod_batch(self.h, _dev(f2), n, stride, stride if frame_len is None else frame_len,
                                              first_symbol, syms_per_frame, _dev(offset), _dev(f_delta), _dev(hk),
                                              hk_stride, _dev(out), nb, _dev(soft)), "rx_demod")
        return (out, soft) if want_soft else out

    # ---------------------------------------------------------------- EXT-9: sc16 input
    def sc16_widen(self, samples: torch.Tensor, scale: float = SC16_DEFAULT_SCALE, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """ofdm_sc16_widen_batch (k_sc16_widen): int16 [n_frames, len, 2] -> complex64 [n_frames, len] (out: rows may be longer)."""
        t = self._sc16(samples)
        n, ln, stride = self._rows(t)
        out = self.empty((n, ln), torch.complex64) if out is None else out
        o2 = out if out.dim() == 2 else out.unsqueeze(0)
        self._ck(self.lib.ofdm_sc16_widen_batch(self.h, _dev(t), n, stride, ln, scale, _dev(o2), o2.stride(0) if n > 1 else max(o2.shape[1], ln)),
                 "sc16_widen")
        return out

    def sc16_narrow(self, samples: torch.Tensor, scale: float = 1.0 / SC16_DEFAULT_SCALE, out: Optional[torch.Tensor] = None):
        """ofdm_sc16_narrow_batch (k_sc16_narrow): complex64 [n_frames, len] -> (int16 [n_frames, len, 2], clipped int32 [n_frames])."""
        x = samples if samples.dim() == 2 else samples.unsqueeze(0)
        if x.dtype != torch.complex64 or x.device != self.device or x.stride(-1) != 1:
            raise OfdmError("expected complex64 rows on the context's device")
        n, ln = x.shape
        out = self.empty((n, ln, 2), torch.int16) if out is None else self._sc16(out)
        clipped = self.empty((n,), torch.int32)
        self._ck(self.lib.ofdm_sc16_narrow_batch(self.h, _dev(x), n, x.stride(0) if n > 1 else ln, ln, scale, _dev(out),
                                                 out.stride(0) // 2 if n > 1 else max(out.shape[1], ln), _dev(clipped)), "sc16_narrow")
        return out, clipped

    def rx_demod_sc16(self, frames: torch.Tensor, syms_per_frame: int, first_symbol: int = 0, offset: Optional[torch.Tensor] = None,
                      f_delta: Optional[torch.Tensor] = None, hk: Optional[torch.Tensor] = None, frame_len: Optional[int] = None,
                      want_soft: bool = False, out: Optional[torch.Tensor] = None, scale: float = SC16_DEFAULT_SCALE):
        """ofdm_rx_demod_sc16_batch: rx_demod of int16 [n_frames, stride, 2]; N = 64 regular streams run k_demod64_sc16."""
        t = self._sc16(frames)
        n, ln, stride = self._rows(t)
        nb = syms_per_frame * self.bytes_per_symbol
        out = self.empty((n, nb), torch.uint8) if out is None else self._u8(out)
        soft = self.empty((n, syms_per_frame * self.data_carriers), torch.complex64) if want_soft else None
        hk_stride = 0
        if hk is not None:
            hk = self._cx(hk)
            hk_stride = self.n_fft if hk.dim() == 2 else 0
            assert hk.shape[-1] == self.n_fft and (hk.dim() == 1 or hk.shape[0] == n)
        self._ck(self.lib.ofdm_rx_demod_sc16_batch(self.h, _dev(t), n, stride, ln if frame_len is None else frame_len, scale, first_symbol,
                                                   syms_per_frame, _dev(offset), _dev(f_delta), _dev(hk), hk_stride, _dev(out), nb,
                                                   _dev(soft)), "rx_demod_sc16")
        return (out, soft) if want_soft else out

    def decode_batch_sc16(self, frames: torch.Tensor, max_symbols: int, n_lags: int = 0, frame_len: Optional[int] = None,
                          scale: float = SC16_DEFAULT_SCALE):
        """ofdm_rx_decode_sc16_batch: decode_batch of int16 captures [n_frames, stride, 2]."""
        t = self._sc16(frames)
        n, ln, stride = self._rows(t)
        ob = self.decode_row_bytes(max_symbols)
        out = self.empty((n, ob), torch.uint8)
        res = {
            "bytes": out, "len": self.empty((n,), torch.int32), "status": self.empty((n,), torch.int32),
            "offset": self.empty((n,), torch.int32), "f_delta": self.empty((n,), torch.float64),
            "metric": self.empty((n,), torch.float32),
        }
        self._ck(self.lib.ofdm_rx_decode_sc16_batch(self.h, _dev(t), n, stride, ln if frame_len is None else frame_len, scale, n_lags,
                                                    max_symbols, _dev(out), ob, _dev(res["len"]), _dev(res["status"]),
                                                    _dev(res["offset"]), _dev(res["f_delta"]), _dev(res["metric"])), "rx_decode_sc16")
        return res

    def decode_host_sc16(self, frames: np.ndarray, max_symbols: int, n_lags: int = 0, frame_len: Optional[int] = None,
                         chunk_frames: int = 0, out: Optional[dict] = None, scale: float = SC16_DEFAULT_SCALE):
        """ofdm_rx_decode_sc16_host: decode_host for a host array [n_frames, stride, 2] of int16 (half the H2D bytes)."""
        x = _sc16_host(frames, "decode_host_sc16")
        n, stride = x.shape[0], x.shape[1]
        ob = self.decode_row_bytes(max_symbols)
        res = out or {"bytes": np.zeros((n, ob), np.uint8), "len": np.zeros(n, np.int32), "status": np.zeros(n, np.int32),
                      "offset": np.zeros(n, np.int32), "f_delta": np.zeros(n, np.float64), "metric": np.zeros(n, np.float32)}
        self._ck(self.lib.ofdm_rx_decode_sc16_host(self.h, _host(x), n, stride, stride if frame_len is None else frame_len, scale, n_lags,
                                                   max_symbols, _host(res["bytes"]), res["bytes"].shape[1], _host(res["len"]),
                                                   _host(res["status"]), _host(res["offset"]), _host(res["f_delta"]),
                                                   _host(res["metric"]), chunk_frames), "rx_decode_sc16_host")
        return res

    def demod_host_sc16(self, frames: np.ndarray, syms_per_frame: int, first_symbol: int = 0, chunk_frames: int = 0,
                        out: Optional[np.ndarray] = None, scale: float = SC16_DEFAULT_SCALE) -> np.ndarray:
        """ofdm_rx_demod_sc16_host: demod_host for a host array [n_frames, stride, 2] of int16 (half the H2D bytes)."""
        x = _sc16_host(frames, "demod_host_sc16")
        n, stride = x.shape[0], x.shape[1]
        nb = syms_per_frame * self.bytes_per_symbol
        out = np.zeros((n, nb), np.uint8) if out is None else out
        self._ck(self.lib.ofdm_rx_demod_sc16_host(self.h, _host(x), n, stride, stride, scale, first_symbol, syms_per_frame, _host(out),
                                                  out.shape[1], chunk_frames), "rx_demod_sc16_host")
        return out

    # ---------------------------------------------------------------- EXT-10: sc16 output, sc16 long captures
    def encode_batch_sc16(self, payload: torch.Tensor, scale: float, out: Optional[torch.Tensor] = None,
                          lens: Optional[torch.Tensor] = None, want_clipped: bool = False):
        """ofdm_tx_encode_sc16_batch: encode_batch writing int16 [n_frames, frame, 2] = sc16_narrow(encode_batch(...), scale) row by row
        (out: rows may be longer, what lies behind the frame is not written).  want_clipped: also the clipped components per frame
        (int32 [n_frames]); a normalised frame's negative peak is not bounded by -1, so a count above 0 says the scale is too large."""
        payload = self._u8(payload)
        n, nbytes = payload.shape
        frame = self.frame_samples(nbytes)
        out = self.empty((n, frame, 2), torch.int16) if out is None else out
        o3 = self._sc16(out)
        if o3.shape[0] != n or o3.shape[1] < frame:
            raise OfdmError("encode_batch_sc16: out must hold n_frames rows of at least frame_samples(payload_bytes) samples")
        if lens is not None:
            lens = lens.to(device=self.device, dtype=torch.int32).contiguous()
            assert lens.numel() == n
        clipped = self.empty((n,), torch.int32) if want_clipped else None
        self._ck(self.lib.ofdm_tx_encode_sc16_batch(self.h, _dev(payload), n, nbytes, _dev(lens), nbytes, scale, _dev(o3),
                                                    self._rows(o3)[2], _dev(clipped)), "tx_encode_sc16")
        return (out, clipped) if want_clipped else out

    def encode_host_sc16(self, payload: np.ndarray, scale: float, lens: Optional[np.ndarray] = None, chunk_frames: int = 0,
                         out: Optional[np.ndarray] = None, want_clipped: bool = False):
        """ofdm_tx_encode_sc16_host: encode_host writing int16 [n_frames, frame (or more), 2] (half the D2H bytes)."""
        pay = np.ascontiguousarray(payload, dtype=np.uint8)
        n, nbytes = pay.shape
        frame = self.frame_samples(nbytes)
        out = np.zeros((n, frame, 2), np.int16) if out is None else out
        if out.dtype != np.int16 or out.ndim != 3 or out.shape[2] != 2 or not out.flags.c_contiguous or out.shape[0] != n:
            raise OfdmError("encode_host_sc16: out must be a contiguous int16 array [n_frames, samples, 2]")
        if lens is not None:
            lens = np.ascontiguousarray(lens, dtype=np.int32)
        clipped = np.zeros(n, np.int32) if want_clipped else None
        self._ck(self.lib.ofdm_tx_encode_sc16_host(self.h, _host(pay), n, nbytes, _host(lens), nbytes, scale, _host(out), out.shape[1],
                                                   _host(clipped), chunk_frames), "tx_encode_sc16_host")
        return (out, clipped) if want_clipped else out

    def decode_long_sc16(self, capture: torch.Tensor, max_symbols: int, scale: float = SC16_DEFAULT_SCALE, lag_lo: int = 0, lag_hi: int = 0,
                         d_hat_known: int = -1):
        """ofdm_rx_decode_long_sc16: decode_long of ONE int16 capture [n, 2] on the device, widened there with `scale`."""
        t = self._sc16(capture)
        if t.shape[0] != 1:
            raise OfdmError("decode_long_sc16: expected one capture [n, 2]")
        ob = self.decode_row_bytes(max_symbols)
        out = self.empty((ob,), torch.uint8)
        ln, st, off, fd, m = C.c_int32(), C.c_int32(), C.c_int64(), C.c_double(), C.c_float()
        self._ck(self.lib.ofdm_rx_decode_long_sc16(self.h, _dev(t), t.shape[1], scale, lag_lo, lag_hi, d_hat_known, max_symbols, _dev(out),
                                                   ob, C.byref(ln), C.byref(st), C.byref(off), C.byref(fd), C.byref(m)), "rx_decode_long_sc16")
        return {"bytes": out, "len": int(ln.value), "status": int(st.value), "offset": int(off.value), "f_delta": float(fd.value),
                "metric": float(m.value)}

    def decode_long_host_sc16(self, capture: np.ndarray, max_symbols: int, scale: float = SC16_DEFAULT_SCALE):
        """ofdm_rx_decode_long_sc16_host: the same from a host array of int16 [n, 2] (pinned_empty() memory is DMA-ed in place)."""
        x = _sc16_host(capture, "decode_long_host_sc16").reshape(-1, 2)
        ob = self.decode_row_bytes(max_symbols)
        out = np.zeros(ob, np.uint8)
        ln, st, off, fd, m = C.c_int32(), C.c_int32(), C.c_int64(), C.c_double(), C.c_float()
        self._ck(self.lib.ofdm_rx_decode_long_sc16_host(self.h, _host(x), x.shape[0], scale, max_symbols, _host(out), ob, C.byref(ln),
                                                        C.byref(st), C.byref(off), C.byref(fd), C.byref(m)), "rx_decode_long_sc16_host")
        return {"bytes": out, "len": int(ln.value), "status": int(st.value), "offset": int(off.value), "f_delta": float(fd.value),
                "metric": float(m.value)}

    def rx_llr(self, frames: torch.Tensor, syms_per_frame: int, first_symbol: int = 0, offset: Optional[torch.Tensor] = None,
               f_delta: Optional[torch.Tensor] = None, hk: Optional[torch.Tensor] = None, frame_len: Optional[int] = None,
               scale: float = SOFT_LLR_SCALE, out: Optional[torch.Tensor] = None, bin_weight: Optional[torch.Tensor] = None) -> torch.Tensor:
        """ofdm_rx_llr_batch: rx_demod with int8 max-log LLRs out -> [n_frames, syms_per_frame * data_carriers * bps], LLR j = bit j
        of the stream rx_demod packs LSB-first (positive = bit 1; definition in include/ofdm_hip.h).
        out (optional): an int8 [n_frames, that many] tensor or view whose rows are contiguous; its row stride (llr_stride) may exceed
        the row, and neither it nor the base needs any alignment.
        bin_weight (optional, EXT-11): float32 [n_fft] (shared) or [n_frames, n_fft] -- ofdm_rx_llr_weighted_batch: the LLR scale of
        bin k is multiplied by the frame's weight at k (noise_bins' q)."""
        frames = self._cx(frames)
        f2 = frames.view(-1, frames.shape[-1])
        n, stride = f2.shape
        nl = syms_per_frame * self.data_carriers * self.modulation
        if out is None:
            out = self.empty((n, nl), torch.int8)
        elif out.dtype != torch.int8 or out.device != self.device or out.shape != (n, nl) or (nl > 1 and out.stride(1) != 1) or \
                (n > 1 and out.stride(0) < nl):
            raise OfdmError("rx_llr: out must be an int8 [n_frames, syms_per_frame * data_carriers * bps] tensor with contiguous rows on the context's device")
        llr_stride = out.stride(0) if n > 1 else nl
        hk_stride = 0
        if hk is not None:
            hk = self._cx(hk)
            hk_stride = self.n_fft if hk.dim() == 2 else 0  # [n_frames, N] per frame, [N] shared
            assert hk.shape[-1] == self.n_fft and (hk.dim() == 1 or hk.shape[0] == n)
        if bin_weight is not None:
            bw = bin_weight
            if bw.dtype != torch.float32 or bw.device != self.device or not bw.is_contiguous() or bw.shape not in ((self.n_fft,), (n, self.n_fft)):
                raise OfdmError("rx_llr: bin_weight must be a contiguous float32 [n_fft] or [n_frames, n_fft] tensor on the context's device")
            self._ck(self.lib.ofdm_rx_llr_weighted_batch(self.h, _dev(f2), n, stride, stride if frame_len is None else frame_len, first_symbol,
                                                         syms_per_frame, _dev(offset), _dev(f_delta), _dev(hk), hk_stride, float(scale),
                                                         _dev(out), llr_stride, _dev(bw), self.n_fft if bw.dim() == 2 else 0), "rx_llr_weighted")
            return out
        self._ck(self.lib.ofdm_rx_llr_batch(self.h, _dev(f2), n, stride, stride if frame_len is None else frame_len, first_symbol,
                                            syms_per_frame, _dev(offset), _dev(f_delta), _dev(hk), hk_stride, float(scale), _dev(out), llr_stride),
                 "rx_llr")
        return out

    def noise_bins(self, frames: torch.Tensor, offset: torch.Tensor, f_delta: Optional[torch.Tensor] = None,
                   status: Optional[torch.Tensor] = None, frame_len: Optional[int] = None) -> dict:
        """ofdm_rx_noise_bins_batch (EXT-11): per frame the noise variance of every received bin from the scatter of the five training
        blocks at offset, and the LLR weight it gives -> {nvar: float32 [n_frames, n_fft] = s_k, weight: float32 [n_frames, n_fft] =
        q_k = mean(s) / s_k where s_k > mean(s), else 1}.  status (optional): frames with status != 0 are not read (s = 0, q = 1), as are
        frames whose training blocks the capture cuts.  Works whatever the context's llr_weight.  Definition: include/ofdm_hip.h,
        tests/noise_weight_ref.py."""
        frames = self._cx(frames)
        f2 = frames.view(-1, frames.shape[-1])
        n, stride = f2.shape
        for name, t, dt in (("offset", offset, torch.int32), ("f_delta", f_delta, torch.float64), ("status", status, torch.int32)):
            if (t is None and name == "offset") or (t is not None and (t.dtype != dt or t.device != self.device or not t.is_contiguous() or t.numel() != n)):
                raise OfdmError(f"noise_bins: {name} must be a contiguous {dt} tensor of n_frames elements on the context's device")
        nvar = self.empty((n, self.n_fft), torch.float32)
        weight = self.empty((n, self.n_fft), torch.float32)
        self._ck(self.lib.ofdm_rx_noise_bins_batch(self.h, _dev(f2), n, stride, stride if frame_len is None else frame_len, _dev(offset),
                                                   _dev(f_delta), _dev(status), _dev(nvar), _dev(weight)), "rx_noise_bins")
        return {"nvar": nvar, "weight": weight}

    def frame_points(self, payload_bytes: int) -> int:
        """Occupied constellation points of a frame of payload_bytes: ceil(8 (16 + coded_len(payload_bytes)) / bps), the 16-byte length
        header included.  Transmit pads the last data symbol with zero points behind them."""
        return -(-8 * (16 + self.coded_len(payload_bytes)) // self.modulation)

    def rx_quality(self, frames: torch.Tensor, syms_per_frame: int, first_symbol: int = 10, n_points=None,
                   offset: Optional[torch.Tensor] = None, f_delta: Optional[torch.Tensor] = None, hk: Optional[torch.Tensor] = None,
                   status: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, frame_len: Optional[int] = None) -> torch.Tensor:
        """ofdm_rx_quality_batch -> float32 [n_frames, QUALITY_FIELDS] (columns Q_*): noise variance, gain, linear SNR and LLR unit from
        the five training blocks, and the decision-directed EVM^2 over the first n_points points of every frame (an int for all frames,
        an int32 tensor per frame, None = no EVM) from data symbol first_symbol on.  status (optional): rows of frames with status != 0
        are 0 and the frames are not read.  Definition: include/ofdm_hip.h, tests/quality_ref.py."""
        frames = self._cx(frames)
        f2 = frames.view(-1, frames.shape[-1])
        n, stride = f2.shape
        if n_points is not None and not isinstance(n_points, torch.Tensor):
            n_points = torch.full((n,), int(n_points), dtype=torch.int32, device=self.device)
        for name, t, dt in (("n_points", n_points, torch.int32), ("offset", offset, torch.int32), ("f_delta", f_delta, torch.float64),
                            ("status", status, torch.int32)):
            if t is not None and (t.dtype != dt or t.device != self.device or not t.is_contiguous() or t.numel() != n):
                raise OfdmError(f"rx_quality: {name} must be a contiguous {dt} tensor of n_frames elements on the context's device")
        if out is None:
            out = self.empty((n, QUALITY_FIELDS), torch.float32)
        elif out.dtype != torch.float32 or out.device != self.device or out.shape != (n, QUALITY_FIELDS) or not out.is_contiguous():
            raise OfdmError("rx_quality: out must be a contiguous float32 [n_frames, QUALITY_FIELDS] tensor on the context's device")
        hk_stride = 0
        if hk is not None:
            hk = self._cx(hk)
            hk_stride = self.n_fft if hk.dim() == 2 else 0  # [n_frames, N] per frame, [N] shared
            assert hk.shape[-1] == self.n_fft and (hk.dim() == 1 or hk.shape[0] == n)
        self._ck(self.lib.ofdm_rx_quality_batch(self.h, _dev(f2), n, stride, stride if frame_len is None else frame_len, first_symbol,
                                                syms_per_frame, _dev(n_points), _dev(offset), _dev(f_delta), _dev(hk), hk_stride,
                                                _dev(status), _dev(out)), "rx_quality")
        return out

    def cfo_wide(self, frames: torch.Tensor, offset: torch.Tensor, f_delta: torch.Tensor, span: int = CFO_WIDE_SPAN,
                 status: Optional[torch.Tensor] = None, frame_len: Optional[int] = None) -> dict:
        """ofdm_cfo_wide_batch: the whole multiples of 2 pi / S the Schmidl-Cox estimate f_delta cannot see, from the five training blocks
        at offset -> {m: int32 [n_frames], f_delta: float64 [n_frames] = f_delta + 2 pi m / S, metric: float32 [n_frames, 2] = the window
        energy of m and the largest among the other hypotheses}.  The f_delta passed in is left as it is.  status (optional): frames with
        status != 0 are not read (m = 0, metrics 0, f_delta unchanged).  Works whatever the context's cfo_mode.  Definition:
        include/ofdm_hip.h, tests/cfo_wide_ref.py."""
        frames = self._cx(frames)
        f2 = frames.view(-1, frames.shape[-1])
        n, stride = f2.shape
        for name, t, dt in (("offset", offset, torch.int32), ("f_delta", f_delta, torch.float64), ("status", status, torch.int32)):
            if (t is None and name != "status") or (t is not None and (t.dtype != dt or t.device != self.device or not t.is_contiguous() or t.numel() != n)):
                raise OfdmError(f"cfo_wide: {name} must be a contiguous {dt} tensor of n_frames elements on the context's device")
        fd = f_delta.clone()
        m = self.empty((n,), torch.int32)
        metric = self.empty((n, 2), torch.float32)
        self._ck(self.lib.ofdm_cfo_wide_batch(self.h, _dev(f2), n, stride, stride if frame_len is None else frame_len, _dev(offset),
                                              _dev(status), int(span), _dev(fd), _dev(m), _dev(metric)), "cfo_wide")
        return {"m": m, "f_delta": fd, "metric": metric}

    def link_quality(self, frames: torch.Tensor, decoded: dict, payload_bytes: Optional[int] = None, n_points=None) -> dict:
        """What the link was like for the frames decode_batch just decoded: `decoded` is the dict it returned for `frames`.  Runs
        estimate_channel with the decode's offset and f_delta (so chest_mode is honoured: under CHEST_WLS the denoised H' equalises and
        weighs) and rx_quality with the decode's status -> tensors over the frames: valid, noise_var, gain, snr_db, llr_unit, evm_db,
        points.  payload_bytes (the frames' payload size; the points are frame_points of it) or n_points (an int or a tensor per frame)
        say which points carry data; without either only the training fields are measured.  snr_db is NaN where valid is 0, evm_db
        where no point was counted.  decode_batch itself is untouched: this is one channel estimate and one more pass over the frames."""
        frames = self._cx(frames)
        f2 = frames.view(-1, frames.shape[-1])
        status = decoded["status"]
        offset = torch.where(status == 0, decoded["offset"], torch.zeros_like(decoded["offset"]))  # (a frame without timing is not read)
        hk = self.estimate_channel(f2, offset, decoded["f_delta"])
        if n_points is None and payload_bytes is not None:
            n_points = self.frame_points(payload_bytes)
        if n_points is None:
            syms = 0
        elif isinstance(n_points, torch.Tensor):
            syms = max(f2.shape[1] // self.S - 10, 0)  # every data symbol a row can hold; only those that hold counted points are walked
        else:
            syms = -(-int(n_points) // self.data_carriers)
        q = self.rx_quality(f2, syms, 10, n_points, offset, decoded["f_delta"], hk, status)
        nan = torch.full_like(q[:, 0], float("nan"))
        return {
            "valid": q[:, Q_VALID] != 0, "noise_var": q[:, Q_NOISE_VAR], "gain": q[:, Q_GAIN],
            "snr_db": torch.where(q[:, Q_VALID] != 0, 10.0 * torch.log10(q[:, Q_SNR]), nan), "llr_unit": q[:, Q_LLR_UNIT],
            "evm_db": torch.where(q[:, Q_POINTS] > 0, 10.0 * torch.log10(q[:, Q_EVM2]), nan), "points": q[:, Q_POINTS],
        }

    # ---------------------------------------------------------------- pipelines
    def encode_batch(self, payload: torch.Tensor, out: Optional[torch.Tensor] = None,
                     lens: Optional[torch.Tensor] = None) -> torch.Tensor:
        """encode (src/transmitter.rs:11-58) for every row of payload [n_frames, payload_bytes] (uint8).
        lens (int32 [n_frames], optional): true payload length of every row (<= payload_bytes); every frame still has
        the slot size of payload_bytes, its unused tail symbols carry pilots only."""
        payload = self._u8(payload)
        n, nbytes = payload.shape
        frame = self.frame_samples(nbytes)
        out = self.empty((n, frame), torch.complex64) if out is None else self._cx(out)
        if lens is not None:
            lens = lens.to(device=self.device, dtype=torch.int32).contiguous()
            assert lens.numel() == n
        self._ck(self.lib.ofdm_tx_encode_batch(self.h, _dev(payload), n, nbytes, _dev(lens), nbytes, _dev(out), out.shape[-1]),
                 "tx_encode")
        return out

    def decode_batch(self, frames: torch.Tensor, max_symbols: int, n_lags: int = 0, frame_len: Optional[int] = None):
        """decode (src/receiver.rs:9-96) for every row of frames [n_frames, stride]; Schmidl-Cox timing/CFO."""
        frames = self._cx(frames)
        f2 = frames.view(-1, frames.shape[-1])
        n, stride = f2.shape
        ob = self.decode_row_bytes(max_symbols)
        out = self.empty((n, ob), torch.uint8)
        res = {
            "bytes": out, "len": self.empty((n,), torch.int32), "status": self.empty((n,), torch.int32),
            "offset": self.empty((n,), torch.int32), "f_delta": self.empty((n,), torch.float64),
            "metric": self.empty((n,), torch.float32),
        }
        self._ck(self.lib.ofdm_rx_decode_batch(self.h, _dev(f2), n, stride, stride if frame_len is None else frame_len,
                                               n_lags, max_symbols, _dev(out), ob, _dev(res["len"]),
                                               _dev(res["status"]), _dev(res["offset"]), _dev(res["f_delta"]),
                                               _dev(res["metric"])), "rx_decode")
        return res

    def llr_combine(self, llr: torch.Tensor, n_branches: int, quality: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None,
                    n_live: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, want_weight: bool = False):
        """ofdm_llr_combine_batch (EXT-7): int8 LLR rows [n_frames * n_branches, n_llr], branch r of frame f being row f * n_branches +
        r (or [n_frames, n_branches, n_llr]) -> the combined rows [n_frames, n_llr]: out[j] = clamp((sum_r q_r L_r[j] + 32) >> 6, +-127)
        with q_r = rint(64 u_r / u_max) from the LLR units of `quality` (float32 rows of QUALITY_FIELDS per branch row; None: every
        branch with status 0 weighs 64).  status, n_live: optional int32 per branch row (a branch with status != 0 is left out; branch
        r counts below n_live only).  llr and out may be views with contiguous rows of any stride and base.  want_weight: also the
        int32 weights per branch row.  Definition: include/ofdm_hip.h, tests/combine_ref.py."""
        if llr.dim() == 3:
            if llr.shape[1] != n_branches or (llr.shape[0] > 1 and llr.stride(0) != n_branches * llr.stride(1)):
                raise OfdmError("llr_combine: a [n_frames, n_branches, n_llr] tensor must have one row stride")
            llr = llr.as_strided((llr.shape[0] * n_branches, llr.shape[2]), (llr.stride(1), llr.stride(2)), llr.storage_offset())
        if llr.dtype != torch.int8 or llr.device != self.device or llr.dim() != 2 or llr.shape[0] % max(n_branches, 1) or \
                (llr.shape[1] > 1 and llr.stride(1) != 1) or (llr.shape[0] > 1 and llr.stride(0) < llr.shape[1]):
            raise OfdmError("llr_combine: llr must be an int8 [n_frames * n_branches, n_llr] tensor with contiguous rows on the context's device")
        rows, nl = llr.shape
        n = rows // max(n_branches, 1)
        for name, t, dt, cnt in (("quality", quality, torch.float32, rows * QUALITY_FIELDS), ("status", status, torch.int32, rows),
                                 ("n_live", n_live, torch.int32, rows)):
            if t is not None and (t.dtype != dt or t.device != self.device or not t.is_contiguous() or t.numel() != cnt):
                raise OfdmError(f"llr_combine: {name} must be a contiguous {dt} tensor of one entry per branch row on the context's device")
        if out is None:
            out = self.empty((n, nl), torch.int8)
        elif out.dtype != torch.int8 or out.device != self.device or out.shape != (n, nl) or (nl > 1 and out.stride(1) != 1) or \
                (n > 1 and out.stride(0) < nl):
            raise OfdmError("llr_combine: out must be an int8 [n_frames, n_llr] tensor with contiguous rows on the context's device")
        weight = self.empty((rows,), torch.int32) if want_weight else None
        self._ck(self.lib.ofdm_llr_combine_batch(self.h, _dev(llr), n, n_branches, llr.stride(0) if rows > 1 else nl, nl, _dev(quality),
                                                 _dev(status), _dev(n_live), _dev(out), out.stride(0) if n > 1 else nl, _dev(weight)),
                 "llr_combine")
        return (out, weight) if want_weight else out

    def decode_combine(self, frames: torch.Tensor, max_symbols: int, n_lags: int = 0, frame_len: Optional[int] = None):
        """ofdm_rx_decode_combine_batch (EXT-7): frames [n_frames, R, stride], R captures of every frame (two antennas, a frame received
        twice) -> one decode per frame from the captures' LLRs combined by link quality.  bytes / len / status: per frame, as
        decode_batch; branch_status, offset, f_delta, metric, weight [n_frames, R] and quality [n_frames, R, QUALITY_FIELDS]: per
        capture.  Modes: ECC_CONV_K7F_* and ECC_LDPC648*, alone or under ECC_RS255 / ECC_FCS."""
        frames = self._cx(frames)
        if frames.dim() != 3:
            raise OfdmError("decode_combine: frames must be [n_frames, n_branches, samples]")
        n, R, stride = frames.shape
        f2 = frames.view(n * R, stride)
        ob = self.decode_row_bytes(max_symbols)
        out = self.empty((n, ob), torch.uint8)
        res = {
            "bytes": out, "len": self.empty((n,), torch.int32), "status": self.empty((n,), torch.int32),
            "branch_status": self.empty((n, R), torch.int32), "offset": self.empty((n, R), torch.int32),
            "f_delta": self.empty((n, R), torch.float64), "metric": self.empty((n, R), torch.float32),
            "weight": self.empty((n, R), torch.int32), "quality": self.empty((n, R, QUALITY_FIELDS), torch.float32),
        }
        self._ck(self.lib.ofdm_rx_decode_combine_batch(self.h, _dev(f2), n, R, stride, stride if frame_len is None else frame_len, n_lags,
                                                       max_symbols, _dev(out), ob, _dev(res["len"]), _dev(res["status"]),
                                                       _dev(res["branch_status"]), _dev(res["offset"]), _dev(res["f_delta"]),
                                                       _dev(res["metric"]), _dev(res["weight"]), _dev(res["quality"])), "rx_decode_combine")
        return res

    def channel_batch(self, tx: torch.Tensor, snr_db: float = 30.0, timing_error: bool = False, seed: int = 1,
                      delay: Optional[torch.Tensor] = None, f_delta: Optional[torch.Tensor] = None,
                      out: Optional[torch.Tensor] = None, span: Optional[int] = None, want_f_delta: bool = False):
        """channel (src/channel.rs:33-74) for every row of tx [n_frames, len]: FIR CHANNEL, optional CFO, pseudo-variance
        noise, seeded (frame f: SplitMix64(seed + f)).  delay (int32) / f_delta (float64) per frame are test-bench
        extensions; span = samples per output row (default len + 63)."""
        tx = self._cx(tx)
        n, ln = tx.shape
        if out is None:
            out = self.empty((n, (ln + 63) if span is None else span), torch.complex64)
        out = self._cx(out)
        assert out.shape[0] == n
        fdo = self.empty((n,), torch.float64) if want_f_delta else None
        if delay is not None:
            delay = delay.to(device=self.device, dtype=torch.int32).contiguous()
        if f_delta is not None:
            f_delta = f_delta.to(device=self.device, dtype=torch.float64).contiguous()
        self._ck(self.lib.ofdm_channel_batch(self.h, _dev(tx), n, ln, ln, float(snr_db), int(timing_error), int(seed) & (2 ** 64 - 1),
                                             _dev(delay), _dev(f_delta), _dev(out), out.shape[-1], out.shape[-1], _dev(fdo)),
                 "channel")
        return (out, fdo) if want_f_delta else out

    # ---------------------------------------------------------------- one long capture (examples/jetson_rx.rs:15-17,84-86)
    def sc_correlate_long(self, capture: torch.Tensor, lag_lo: int = 0, lag_hi: int = 0, slice_lags: int = 0):
        """ofdm_sc_correlate_long: the Schmidl-Cox detection of ONE capture whose first crossing lies in [lag_lo, lag_hi)
        (lag_hi = 0: up to the last lag), searched as a batch of overlapping slices -> (d_hat or -1, f_delta, metric)."""
        x = self._cx(capture).reshape(-1)
        d, fd, m = C.c_int64(), C.c_double(), C.c_float()
        self._ck(self.lib.ofdm_sc_correlate_long(self.h, _dev(x), x.numel(), lag_lo, lag_hi, slice_lags, C.byref(d), C.byref(fd),
                                                 C.byref(m)), "sc_correlate_long")
        return int(d.value), float(fd.value), float(m.value)

    def _scan_result(self, call, what: str, lag_lo: int, holdoff: int, max_det: int) -> dict:
        cap = max(int(max_det), 1)
        d1, dh = np.zeros(cap, np.int64), np.zeros(cap, np.int64)
        fd, m = np.zeros(cap, np.float64), np.zeros(cap, np.float32)
        nd, more = C.c_int64(), C.c_int32()
        self._ck(call(_host(d1), _host(dh), _host(fd), _host(m), C.byref(nd), C.byref(more)), what)
        n = int(nd.value)
        lo = np.concatenate([[int(lag_lo)], d1[:n] + int(holdoff)]).astype(np.int64)
        return {"d1": d1[:n], "d_hat": dh[:n], "f_delta": fd[:n], "metric": m[:n], "lag_lo": lo[:n], "next_lag_lo": int(lo[n]),
                "more": bool(more.value)}

    def default_holdoff(self) -> int:
        """The holdoff of the shortest frame (a header and one data symbol): 11 S - W, at least 1."""
        return max(11 * self.S - self.params.sync_window_reps * self.S, 1)

    def sc_scan_long(self, capture: torch.Tensor, holdoff: int, max_det: int, lag_lo: int = 0, lag_hi: int = 0) -> dict:
        """ofdm_sc_scan_long (EXT-12): EVERY Schmidl-Cox detection of ONE capture whose first crossing lies in [lag_lo, lag_hi), in one
        pass: detection k + 1 is the first crossing at or after d1[k] + holdoff.  -> dict of numpy arrays d1, d_hat (int64), f_delta,
        metric and lag_lo (where the search for detection k started: decode_long(lag_lo=lag_lo[k]) decodes packet k), next_lag_lo
        (where a further scan would start) and more (max_det stopped the scan while a further detection exists)."""
        x = self._cx(capture).reshape(-1)
        return self._scan_result(lambda *out: self.lib.ofdm_sc_scan_long(self.h, _dev(x), x.numel(), lag_lo, lag_hi, holdoff, max_det, *out),
                                 "sc_scan_long", lag_lo, holdoff, max_det)

    def sc_scan_long_host(self, capture: np.ndarray, holdoff: int, max_det: int, lag_lo: int = 0, lag_hi: int = 0) -> dict:
        """ofdm_sc_scan_long_host: the same from a host array of complex64 (pinned_empty() memory is DMA-ed in place)."""
        x = np.ascontiguousarray(capture, dtype=np.complex64).reshape(-1)
        return self._scan_result(lambda *out: self.lib.ofdm_sc_scan_long_host(self.h, _host(x), x.size, lag_lo, lag_hi, holdoff, max_det, *out),
                                 "sc_scan_long_host", lag_lo, holdoff, max_det)

    def decode_long(self, capture: torch.Tensor, max_symbols: int, lag_lo: int = 0, lag_hi: int = 0, d_hat_known: int = -1):
        """ofdm_rx_decode_long: decode (src/receiver.rs:9-96) of ONE long capture on the device -> dict(bytes, len, status, offset,
        f_delta, metric), the result of decode_batch on the whole capture as a single frame."""
        x = self._cx(capture).reshape(-1)
        ob = self.decode_row_bytes(max_symbols)
        out = self.empty((ob,), torch.uint8)
        ln, st, off, fd, m = C.c_int32(), C.c_int32(), C.c_int64(), C.c_double(), C.c_float()
        self._ck(self.lib.ofdm_rx_decode_long(self.h, _dev(x), x.numel(), lag_lo, lag_hi, d_hat_known, max_symbols, _dev(out), ob,
                                              C.byref(ln), C.byref(st), C.byref(off), C.byref(fd), C.byref(m)), "rx_decode_long")
        return {"bytes": out, "len": int(ln.value), "status": int(st.value), "offset": int(off.value), "f_delta": float(fd.value),
                "metric": float(m.value)}

    def decode_long_host(self, capture: np.ndarray, max_symbols: int):
        """ofdm_rx_decode_long_host: the same from a host array of complex64 (pinned_empty() memory is DMA-ed in place)."""
        x = np.ascontiguousarray(capture, dtype=np.complex64).reshape(-1)
        ob = self.decode_row_bytes(max_symbols)
        out = np.zeros(ob, np.uint8)
        ln, st, off, fd, m = C.c_int32(), C.c_int32(), C.c_int64(), C.c_double(), C.c_float()
        self._ck(self.lib.ofdm_rx_decode_long_host(self.h, _host(x), x.size, max_symbols, _host(out), ob, C.byref(ln), C.byref(st),
                                                   C.byref(off), C.byref(fd), C.byref(m)), "rx_decode_long_host")
        return {"bytes": out, "len": int(ln.value), "status": int(st.value), "offset": int(off.value), "f_delta": float(fd.value),
                "metric": float(m.value)}

    def decode_packets(self, capture: torch.Tensor, det: dict, max_symbols: int, out_stride: Optional[int] = None) -> dict:
        """ofdm_rx_decode_packets (EXT-13): every detection of `det` (sc_scan_long's dict, or any dict of numpy d_hat / f_delta / metric)
        through ONE run of the receive chain -> dict of device tensors bytes [n_det, out_stride], len, status (int32), offset (int64,
        into the capture), f_delta (the value the chain derotated with) and metric (the scan's, bit for bit).  Asynchronous."""
        x = self._cx(capture).reshape(-1)
        dh = np.ascontiguousarray(det["d_hat"], dtype=np.int64)
        fd = np.ascontiguousarray(det["f_delta"], dtype=np.float64)
        m = np.ascontiguousarray(det["metric"], dtype=np.float32)
        n = dh.size
        if fd.size != n or m.size != n:
            raise OfdmError("decode_packets: d_hat, f_delta and metric must have one entry per detection")
        ob = self.decode_row_bytes(max_symbols) if out_stride is None else int(out_stride)
        res = {"bytes": self.empty((n, ob), torch.uint8), "len": self.empty((n,), torch.int32), "status": self.empty((n,), torch.int32),
               "offset": self.empty((n,), torch.int64), "f_delta": self.empty((n,), torch.float64), "metric": self.empty((n,), torch.float32)}
        self._ck(self.lib.ofdm_rx_decode_packets(self.h, _dev(x), x.numel(), n, _host(dh), _host(fd), _host(m), max_symbols, _dev(res["bytes"]), ob,
                                                 _dev(res["len"]), _dev(res["status"]), _dev(res["offset"]), _dev(res["f_delta"]),
                                                 _dev(res["metric"])), "rx_decode_packets")
        return res

    def decode_all_host(self, capture: np.ndarray, holdoff: int, max_det: int, max_symbols: int, lag_lo: int = 0, lag_hi: int = 0) -> dict:
        """ofdm_rx_decode_all_long_host (EXT-13): upload, scan and batched decode of a host array of complex64 (pinned_empty() memory is
        DMA-ed in place) -> dict of numpy arrays: bytes [n_det, row], len, status, offset, f_delta, metric per packet and the scan's d1,
        d_hat, lag_lo, next_lag_lo, more.  Two synchronisations whatever the packet count."""
        x = np.ascontiguousarray(capture, dtype=np.complex64).reshape(-1)
        cap = max(int(max_det), 1)
        ob = self.decode_row_bytes(max_symbols)
        out = np.zeros((cap, ob), np.uint8)
        ln, st, off = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int64)
        fd, m = np.zeros(cap, np.float64), np.zeros(cap, np.float32)
        d1, dh = np.zeros(cap, np.int64), np.zeros(cap, np.int64)
        nd, more = C.c_int64(), C.c_int32()
        self._ck(self.lib.ofdm_rx_decode_all_long_host(self.h, _host(x), x.size, lag_lo, lag_hi, holdoff, max_det, max_symbols, _host(out), ob,
                                                       _host(ln), _host(st), _host(off), _host(fd), _host(m), _host(d1), _host(dh),
                                                       C.byref(nd), C.byref(more)), "rx_decode_all_long_host")
        n = int(nd.value)
        lo = np.concatenate([[int(lag_lo)], d1[:n] + int(holdoff)]).astype(np.int64)
        return {"bytes": out[:n], "len": ln[:n], "status": st[:n], "offset": off[:n], "f_delta": fd[:n], "metric": m[:n], "d1": d1[:n],
                "d_hat": dh[:n], "lag_lo": lo[:n], "next_lag_lo": int(lo[n]), "more": bool(more.value)}

    def stream(self, max_symbols: int, holdoff: Optional[int] = None, max_chunk: int = 65536, first_sample: int = 0,
               dc_blocks: int = 0, ddc=None) -> "Stream":
        """ofdm_stream_create (EXT-14): a streaming receiver on this context -- push chunks as a radio hands them over, get every packet
        exactly once, bit for bit the packets of decode_all_host on the concatenation.  holdoff None: default_holdoff().
        dc_blocks (EXT-15, 0 = off): the DC blocker in front of the window; the packets are then those of decode_all_host on
        dc_block_host(concatenation, dc_blocks).
        ddc (EXT-16, None = off): (decim, f0, taps) -- the down-converter in front of everything else: pushes are input-rate samples
        with the signal at f0 cycles per sample, the packets are those of decode_all_host on ddc_host(concatenation, decim,
        ddc_inc_for(f0), taps) (taps None: ddc_design(decim)); holdoff, first_sample and every offset are in OUTPUT samples."""
        import weakref

        s = Stream(self, max_symbols, self.default_holdoff() if holdoff is None else holdoff, max_chunk, first_sample)
        if not hasattr(self, "_streams"):
            self._streams = weakref.WeakSet()
        self._streams.add(s)
        if dc_blocks:
            s.set_dc_block(dc_blocks)
        if ddc is not None:
            decim, f0, taps = (tuple(ddc) + (None, None))[:3]
            s.set_ddc(decim, ddc_inc_for(f0 or 0.0), taps)
        return s

    def ddc(self, decim: int, phase_inc: int = 0, taps=None, max_chunk: int = 1 << 20) -> "Ddc":
        """ofdm_ddc_create (EXT-16): a stateful down-converter on device buffers -- the outputs of its pushes, concatenated, are ddc_host
        of the concatenated inputs bit for bit.  taps None: ddc_design(decim).  Close it before its context."""
        import weakref

        f = Ddc(self, decim, phase_inc, _ddc_taps(decim, taps), max_chunk)
        if not hasattr(self, "_streams"):
            self._streams = weakref.WeakSet()
        self._streams.add(f)
        return f

    def ddc_once(self, samples, decim: int, phase_inc: int = 0, taps=None, scale: Optional[float] = None) -> torch.Tensor:
        """One shot: a whole stream (complex64, or int16 [n, 2] with scale=) through a fresh down-converter -> complex64 device tensor."""
        with self.ddc(decim, phase_inc, taps) as f:
            return f.push(samples, scale=scale)

    def dc_filter(self, blocks: Optional[int] = None, max_chunk: int = 1 << 20) -> "DcBlock":
        """ofdm_dcblock_create (EXT-15): a stateful DC blocker on device buffers -- its pushes, concatenated, are dc_block_host of the
        concatenated inputs bit for bit.  blocks None: dc_block_default(n_fft).  Close it before its context."""
        import weakref

        f = DcBlock(self, dc_block_default(self.params.n_fft) if blocks is None else blocks, max_chunk)
        if not hasattr(self, "_streams"):
            self._streams = weakref.WeakSet()
        self._streams.add(f)
        return f

    def dc_block(self, samples, blocks: Optional[int] = None, scale: Optional[float] = None) -> torch.Tensor:
        """One shot: a whole stream (complex64, or int16 [n, 2] with scale=) through a fresh DC blocker -> complex64 device tensor."""
        with self.dc_filter(blocks) as f:
            return f.push(samples, scale=scale)

    # ---------------------------------------------------------------- host buffers (H2D / kernels / D2H pipelined in the library)
    def decode_host(self, frames: np.ndarray, max_symbols: int, n_lags: int = 0, frame_len: Optional[int] = None,
                    chunk_frames: int = 0, out: Optional[dict] = None):
        """ofdm_rx_decode_host: decode_batch for a host array [n_frames, stride] of complex64 -> dict of host arrays."""
        x = frames if frames.dtype == np.complex64 and frames.flags.c_contiguous else np.ascontiguousarray(frames, dtype=np.complex64)
        n, stride = x.shape
        ob = self.decode_row_bytes(max_symbols)
        res = out or {"bytes": np.zeros((n, ob), np.uint8), "len": np.zeros(n, np.int32), "status": np.zeros(n, np.int32),
                      "offset": np.zeros(n, np.int32), "f_delta": np.zeros(n, np.float64), "metric": np.zeros(n, np.float32)}
        self._ck(self.lib.ofdm_rx_decode_host(self.h, _host(x), n, stride, stride if frame_len is None else frame_len, n_lags,
                                              max_symbols, _host(res["bytes"]), res["bytes"].shape[1], _host(res["len"]),
                                              _host(res["status"]), _host(res["offset"]), _host(res["f_delta"]), _host(res["metric"]),
                                              chunk_frames), "rx_decode_host")
        return res

    def demod_host(self, frames: np.ndarray, syms_per_frame: int, first_symbol: int = 0, chunk_frames: int = 0,
                   out: Optional[np.ndarray] = None) -> np.ndarray:
        """ofdm_rx_demod_host: rx_demod of regular streams for a host array [n_frames, stride] -> uint8 [n_frames, bytes]."""
        x = frames if frames.dtype == np.complex64 and frames.flags.c_contiguous else np.ascontiguousarray(frames, dtype=np.complex64)
        n, stride = x.shape
        nb = syms_per_frame * self.bytes_per_symbol
        out = np.zeros((n, nb), np.uint8) if out is None else out
        self._ck(self.lib.ofdm_rx_demod_host(self.h, _host(x), n, stride, stride, first_symbol, syms_per_frame, _host(out),
                                             out.shape[1], chunk_frames), "rx_demod_host")
        return out

    def encode_host(self, payload: np.ndarray, lens: Optional[np.ndarray] = None, chunk_frames: int = 0,
                    out: Optional[np.ndarray] = None) -> np.ndarray:
        """ofdm_tx_encode_host: encode_batch for a host array [n_frames, payload_bytes] of uint8 -> complex64 [n_frames, frame]."""
        pay = np.ascontiguousarray(payload, dtype=np.uint8)
        n, nbytes = pay.shape
        frame = self.frame_samples(nbytes)
        out = np.zeros((n, frame), np.complex64) if out is None else out
        if lens is not None:
            lens = np.ascontiguousarray(lens, dtype=np.int32)
        self._ck(self.lib.ofdm_tx_encode_host(self.h, _host(pay), n, nbytes, _host(lens), nbytes, _host(out), out.shape[1],
                                              chunk_frames), "tx_encode_host")
        return out

    def use_own_stream(self):
        """ofdm_use_own_stream: a non-blocking stream owned by this context (several contexts side by side on one device)."""
        self._ck(self.lib.ofdm_use_own_stream(self.h), "ofdm_use_own_stream")

    def hbm_read_probe(self, samples: torch.Tensor, pattern: int = 0):
        """Measurement helper: read-only pass over a buffer of 80-sample symbols in the demod kernel's access pattern (0),
        over whole symbols (1) or with unit-stride 16-byte loads (2)."""
        samples = self._cx(samples)
        self._ck(self.lib.ofdm_hbm_read_probe(self.h, _dev(samples), samples.numel() // 80, pattern), "hbm_read_probe")

    # event timing on the context's stream (bench.py)
    def timer_start(self):
        self._ck(self.lib.ofdm_timer_start(self.h), "timer_start")

    def timer_stop_ms(self) -> float:
        ms = C.c_float()
        self._ck(self.lib.ofdm_timer_stop_ms(self.h, C.byref(ms)), "timer_stop")
        return float(ms.value)


class DcBlock:
    """`ofdm_dcblock` (EXT-15, include/ofdm_hip.h "a DC blocker in front of detection"): Context.dc_filter(...) makes one.  Blocks of 64
    samples aligned at the first sample pushed; every sample leaves less the mean of the `blocks` complete blocks in front of its own
    block.  However the stream is cut into pushes, the outputs concatenated are dc_block_host of the inputs concatenated."""

    def __init__(self, ctx: "Context", blocks: int, max_chunk: int):
        self.ctx, self.lib = ctx, ctx.lib
        h = C.c_void_p()
        ctx._ck(self.lib.ofdm_dcblock_create(C.byref(h), ctx.h, int(blocks), int(max_chunk)), "ofdm_dcblock_create")
        self.h = h
        self.blocks = int(blocks)

    def close(self):
        if getattr(self, "h", None):
            self.lib.ofdm_dcblock_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def push(self, samples, scale: Optional[float] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """ofdm_dcblock_push / _push_sc16: complex64 samples (a device tensor, or a host array that is uploaded), or int16 [n, 2] with
        scale=, -> the filtered complex64 device tensor (out=: written there; it may not overlap the input).  Asynchronous."""
        ctx = self.ctx
        t = samples if isinstance(samples, torch.Tensor) else ctx.to_device(np.asarray(samples))
        if t.dtype == torch.int16:
            if scale is None:
                raise OfdmError("DcBlock.push: int16 samples need scale=")
            t = ctx._sc16(t).reshape(-1, 2)
            n = t.shape[0]
            out = ctx.empty((n,), torch.complex64) if out is None else ctx._cx(out)
            ctx._ck(self.lib.ofdm_dcblock_push_sc16(self.h, _dev(t), n, float(scale), _dev(out)), "ofdm_dcblock_push_sc16")
            return out
        t = ctx._cx(t).reshape(-1)
        out = ctx.empty((t.numel(),), torch.complex64) if out is None else ctx._cx(out)
        ctx._ck(self.lib.ofdm_dcblock_push(self.h, _dev(t), t.numel(), _dev(out)), "ofdm_dcblock_push")
        return out

    def reset(self):
        self.ctx._ck(self.lib.ofdm_dcblock_reset(self.h), "ofdm_dcblock_reset")

    def state(self) -> dict:
        """ofdm_dcblock_state -> total (samples pushed since create / reset), blocks"""
        t, m = C.c_int64(), C.c_int32()
        self.ctx._ck(self.lib.ofdm_dcblock_state(self.h, C.byref(t), C.byref(m)), "ofdm_dcblock_state")
        return {"total": int(t.value), "blocks": int(m.value)}


class Ddc:
    """`ofdm_ddc_handle` (EXT-16, include/ofdm_hip.h "a digital down-converter"): Context.ddc(...) makes one.  Mix by the two-level
    20-bit rotor, filter by real taps, keep every decim-th sample; however the stream is cut into pushes, the outputs concatenated are
    ddc_host of the inputs concatenated."""

    def __init__(self, ctx: "Context", decim: int, phase_inc: int, taps: np.ndarray, max_chunk: int):
        self.ctx, self.lib = ctx, ctx.lib
        h = C.c_void_p()
        self.decim, self.phase_inc, self.n_taps = int(decim), int(phase_inc) % DDC_PHASE_MOD, int(taps.size)
        ctx._ck(self.lib.ofdm_ddc_create(C.byref(h), ctx.h, self.decim, self.phase_inc, _host(taps), self.n_taps, int(max_chunk)),
                "ofdm_ddc_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.ofdm_ddc_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def push(self, samples, scale: Optional[float] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """ofdm_ddc_push / _push_sc16: complex64 samples (a device tensor, or a host array that is uploaded), or int16 [n, 2] with
        scale=, -> the converted complex64 device tensor, as long as this push gave outputs (out=: written from its start; it may not
        overlap the input and must hold them).  Asynchronous."""
        ctx = self.ctx
        t = samples if isinstance(samples, torch.Tensor) else ctx.to_device(np.asarray(samples))
        sc16 = t.dtype == torch.int16
        if sc16:
            if scale is None:
                raise OfdmError("Ddc.push: int16 samples need scale=")
            t = ctx._sc16(t).reshape(-1, 2)
            n = t.shape[0]
        else:
            t = ctx._cx(t).reshape(-1)
            n = t.numel()
        st = self.state()
        want = ddc_out_len(st["total_in"] + n, self.decim, self.n_taps) - st["total_out"]
        out = ctx.empty((want,), torch.complex64) if out is None else ctx._cx(out).reshape(-1)
        got = C.c_int64()
        if sc16:
            ctx._ck(self.lib.ofdm_ddc_push_sc16(self.h, _dev(t), n, float(scale), _dev(out), out.numel(), C.byref(got)), "ofdm_ddc_push_sc16")
        else:
            ctx._ck(self.lib.ofdm_ddc_push(self.h, _dev(t), n, _dev(out), out.numel(), C.byref(got)), "ofdm_ddc_push")
        return out[: int(got.value)]

    def reset(self):
        self.ctx._ck(self.lib.ofdm_ddc_reset(self.h), "ofdm_ddc_reset")

    def state(self) -> dict:
        """ofdm_ddc_state -> total_in (samples pushed since create / reset), total_out (samples given)"""
        a, b = C.c_int64(), C.c_int64()
        self.ctx._ck(self.lib.ofdm_ddc_state(self.h, C.byref(a), C.byref(b)), "ofdm_ddc_state")
        return {"total_in": int(a.value), "total_out": int(b.value)}


class Stream:
    """`ofdm_stream` (EXT-14, include/ofdm_hip.h "a streaming receiver"): Context.stream(...) makes one.  However the samples are cut into
    pushes, the packets delivered are those of Context.decode_all_host on the concatenation, each exactly once; packet k arrives with the
    first push after which d1_k + horizon samples are there, or with the flush.  Close it before its context."""
    FIELDS = ("len", "status", "offset", "f_delta", "metric", "d1", "d_hat")

    def __init__(self, ctx: Context, max_symbols: int, holdoff: int, max_chunk: int, first_sample: int = 0):
        self.ctx, self.lib = ctx, ctx.lib
        self.max_symbols, self.holdoff, self.max_chunk = int(max_symbols), int(holdoff), int(max_chunk)
        h = C.c_void_p()
        ctx._ck(self.lib.ofdm_stream_create(C.byref(h), ctx.h, self.max_symbols, self.holdoff, self.max_chunk, int(first_sample)),
                "ofdm_stream_create")
        self.h = h
        self.row_bytes = ctx.decode_row_bytes(self.max_symbols)
        self.horizon = ctx.params.sync_window_reps * ctx.S + (10 + self.max_symbols) * ctx.S + 2

    def close(self):
        if getattr(self, "h", None):
            self.lib.ofdm_stream_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, samples, sc16_scale, flush: bool, max_pkt: int) -> dict:
        cap = max(int(max_pkt), 1)
        ob = max(self.row_bytes, 1)
        out = np.zeros((cap, ob), np.uint8)
        ln, st = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        off, d1, dh = np.zeros(cap, np.int64), np.zeros(cap, np.int64), np.zeros(cap, np.int64)
        fd, m = np.zeros(cap, np.float64), np.zeros(cap, np.float32)
        nd, more = C.c_int64(), C.c_int32()
        tail = (int(bool(flush)), int(max_pkt), _host(out), ob, _host(ln), _host(st), _host(off), _host(fd), _host(m), _host(d1), _host(dh),
                C.byref(nd), C.byref(more))
        if samples is None:
            rc = self.lib.ofdm_stream_push(self.h, None, 0, *tail)
        elif np.asarray(samples).dtype == np.int16:
            a = _sc16_host(samples, "Stream.push").reshape(-1, 2)
            if sc16_scale is None:
                raise OfdmError("Stream.push: int16 samples need sc16_scale=")
            rc = self.lib.ofdm_stream_push_sc16(self.h, _host(a), a.shape[0], float(sc16_scale), *tail)
        else:
            x = np.ascontiguousarray(samples, dtype=np.complex64).reshape(-1)
            rc = self.lib.ofdm_stream_push(self.h, _host(x), x.size, *tail)
        self.ctx._ck(rc, "ofdm_stream_push")
        n = int(nd.value)
        return {"bytes": out[:n], "len": ln[:n], "status": st[:n], "offset": off[:n], "f_delta": fd[:n], "metric": m[:n], "d1": d1[:n],
                "d_hat": dh[:n], "more": bool(more.value)}

    def push(self, samples, flush: bool = False, max_pkt: int = 64, sc16_scale: Optional[float] = None) -> dict:
        """ofdm_stream_push / ofdm_stream_push_sc16: a complex64 array goes to the fc32 form, an int16 array of shape [n, 2] with
        sc16_scale= to the sc16 form; None (or an empty array) pushes nothing.  -> the dict of numpy arrays decode_all_host returns
        (bytes, len, status, offset, f_delta, metric, d1, d_hat per packet delivered by THIS push) and more: packets remain beyond max_pkt
        -- push(None, flush, max_pkt) drains them."""
        return self._call(samples, sc16_scale, flush, max_pkt)

    def push_all(self, samples, flush: bool = False, sc16_scale: Optional[float] = None, max_pkt: int = 64) -> dict:
        """push, then drained through `more`: everything this push made deliverable, in one dict"""
        parts = [self.push(samples, flush, max_pkt, sc16_scale)]
        while parts[-1]["more"]:
            parts.append(self.push(None, flush, max_pkt))
        res = {k: np.concatenate([p[k] for p in parts]) for k in ("bytes",) + self.FIELDS}
        res["more"] = False
        return res

    def flush(self, max_pkt: int = 64) -> dict:
        """every remaining detection, a last frame cut by the end of the stream included; the stream is ended until reset()"""
        return self.push_all(None, True, max_pkt=max_pkt)

    def reset(self, first_sample: int = 0):
        self.ctx._ck(self.lib.ofdm_stream_reset(self.h, int(first_sample)), "ofdm_stream_reset")

    def set_dc_block(self, blocks: int):
        """ofdm_stream_set_dc_block (EXT-15): the DC blocker in front of the window, 0 = off; only before the first sample (or right
        after reset(), which keeps the setting and clears the filter's history)"""
        self.ctx._ck(self.lib.ofdm_stream_set_dc_block(self.h, int(blocks)), "ofdm_stream_set_dc_block")

    def get_dc_block(self) -> int:
        m = C.c_int32()
        self.ctx._ck(self.lib.ofdm_stream_get_dc_block(self.h, C.byref(m)), "ofdm_stream_get_dc_block")
        return int(m.value)

    def set_ddc(self, decim: int, phase_inc: int = 0, taps=None):
        """ofdm_stream_set_ddc (EXT-16): the down-converter in front of everything else, decim 0 = off; taps None: the default design;
        only before the first sample (or right after reset(), which keeps the setting and clears the history)"""
        if not decim:
            self.ctx._ck(self.lib.ofdm_stream_set_ddc(self.h, 0, 0, None, 0), "ofdm_stream_set_ddc")
            return
        h = None if taps is None else np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        self.ctx._ck(self.lib.ofdm_stream_set_ddc(self.h, int(decim), int(phase_inc) % DDC_PHASE_MOD, _host(h), 0 if h is None else h.size),
                     "ofdm_stream_set_ddc")

    def get_ddc(self) -> dict:
        """ofdm_stream_get_ddc -> decim (0 = off), phase_inc, n_taps"""
        d, i, t = C.c_int32(), C.c_int32(), C.c_int32()
        self.ctx._ck(self.lib.ofdm_stream_get_ddc(self.h, C.byref(d), C.byref(i), C.byref(t)), "ofdm_stream_get_ddc")
        return {"decim": int(d.value), "phase_inc": int(i.value), "n_taps": int(t.value)}

    def state(self) -> dict:
        """ofdm_stream_state -> total (samples pushed), kept_from (first sample the window keeps), next_lag (where the walk resumes),
        ended; all stream-relative"""
        t, k, lo, e = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int32()
        self.ctx._ck(self.lib.ofdm_stream_state(self.h, C.byref(t), C.byref(k), C.byref(lo), C.byref(e)), "ofdm_stream_state")
        return {"total": int(t.value), "kept_from": int(k.value), "next_lag": int(lo.value), "ended": bool(e.value)}


def _packet_dicts(res: dict):
    for k in range(len(res["status"])):
        ok = int(res["status"][k]) == FRAME_OK
        yield {"bytes": bytes(res["bytes"][k, : max(int(res["len"][k]), 0)]) if ok else b"", "status": int(res["status"][k]),
               "offset": int(res["offset"][k]), "f_delta": float(res["f_delta"][k]), "metric": float(res["metric"][k]),
               "d1": int(res["d1"][k]), "d_hat": int(res["d_hat"][k])}


def receive_stream(chunks, max_symbols: int, guard_bands: bool = False, modulation: int = BPSK, n_fft: int = 64, ecc: int = ECC_NONE,
                   holdoff: Optional[int] = None, max_chunk: int = 65536, first_sample: int = 0, sc16_scale: Optional[float] = None,
                   dc_blocks: int = 0, ddc=None, **kw):
    """A generator over an iterable of chunks (complex64 arrays, or int16 [n, 2] arrays with sc16_scale=): yields one dict per packet
    (bytes, status, offset, f_delta, metric, d1, d_hat) as soon as the stream commits it, and flushes when the iterable ends.
    dc_blocks (EXT-15, 0 = off): the DC blocker in front of the stream's window.
    ddc (EXT-16, None = off): (decim, f0, taps) -- the chunks are input-rate samples, down-converted in front of everything else."""
    ctx = _ctx(n_fft, modulation, guard_bands, ecc, **kw)
    with ctx.stream(max_symbols, holdoff, max_chunk, first_sample, dc_blocks=dc_blocks, ddc=ddc) as s:
        for chunk in chunks:
            yield from _packet_dicts(s.push_all(chunk, sc16_scale=sc16_scale))
        yield from _packet_dicts(s.flush())


# -------------------------------------------------------------------- reference-shaped free functions
_CTX_CACHE = {}


def _ctx_key(n_fft, modulation, guard_bands, ecc=ECC_NONE, _replica: int = 0, **kw) -> tuple:
    """The cache key of _ctx, a pure function of its arguments.  Explicit `preamble` / `training` tables are inputs of the context
    (ofdm_create), so they are keyed by value: their complex128 bytes and shape, as Context hands them to the library.  Two different
    tables get two contexts, the same table (whatever object or dtype carries it) reuses one; None is the default table."""
    items = []
    for k, v in sorted(kw.items()):
        if k in ("preamble", "training") and v is not None:
            a = np.ascontiguousarray(v, dtype=np.complex128)
            v = (a.shape, a.tobytes())
        elif k == "tuning" and v is not None:
            v = tuple(sorted(dict(v).items()))
        items.append((k, v))
    return (n_fft, modulation, bool(guard_bands), ecc, _replica, tuple(items))


def _ctx(n_fft, modulation, guard_bands, ecc=ECC_NONE, _replica: int = 0, **kw) -> Context:
    """One cached context per parameter set (and replica index): the free functions never pay ofdm_create -- table uploads,
    workspace growth -- more than once."""
    key = _ctx_key(n_fft, modulation, guard_bands, ecc, _replica, **kw)
    if key not in _CTX_CACHE:
        _CTX_CACHE[key] = Context(n_fft=n_fft, modulation=modulation, guard_bands=guard_bands, ecc=ecc, **kw)
    return _CTX_CACHE[key]


def _with_fcs(ecc: int, fcs: bool) -> int:
    return ecc + ECC_FCS if fcs and ecc < ECC_FCS else ecc


_FRAME_ERRORS = {FRAME_NOSYNC: "no preamble found", FRAME_HEADER: "no length header decoded",
                 FRAME_UNCORRECTABLE: "uncorrectable block (Reed-Solomon: the reference returns None; LDPC: a code word did not converge)",
                 FRAME_FCS: "frame check failed: the payload is damaged",
                 FRAME_BADTIMING: "timing offset outside the capture (the reference panics in split_off)"}


def encode(data: bytes, guard_bands: Optional[bool] = None, modulation: Optional[int] = None, n_fft: int = 64,
           ecc: int = ECC_NONE, fcs: bool = False, sc16_scale: Optional[float] = None, **kw) -> np.ndarray:
    """`ofdm::encode!(data, guard_bands, modulation)` (src/transmitter.rs:10-58): bytes -> Vec<Complex64>.
    Defaults as the reference: guard_bands=false, modulation=Bpsk.  fcs: the CRC-32 frame check around the payload (ecc + ECC_FCS).
    sc16_scale: the frame as sc16 for a DAC (EXT-10) -- an int16 array [n, 2] = sc16_narrow(frame, sc16_scale)[0], made on the device."""
    ctx = _ctx(n_fft, BPSK if modulation is None else modulation, bool(guard_bands), _with_fcs(ecc, fcs), **kw)
    pay = torch.frombuffer(bytearray(data) if len(data) else bytearray(1), dtype=torch.uint8)[: len(data)]
    pay = pay.reshape(1, len(data)).to(ctx.device)
    if sc16_scale is not None:
        q = ctx.encode_batch_sc16(pay, sc16_scale)
        ctx.synchronize()
        return q[0].cpu().numpy()
    frames = ctx.encode_batch(pay)
    ctx.synchronize()
    return frames[0].cpu().numpy().astype(np.complex128)


def channel(transmission, snr: Optional[float] = None, timing_error: Optional[bool] = None, seed: int = 1) -> np.ndarray:
    """`ofdm::channel!(transmission, snr, timing_error)` (src/channel.rs:32-74) on the GPU, seeded (the reference's
    thread_rng is not reproducible).  Defaults as the reference: snr 30 dB, timing_error false."""
    ctx = _ctx(64, BPSK, False)
    x = ctx.to_device(np.asarray(transmission)).reshape(1, -1)
    y = ctx.channel_batch(x, 30.0 if snr is None else snr, bool(timing_error), seed)
    ctx.synchronize()
    return y[0].cpu().numpy().astype(np.complex128)


def decode(samples, guard_bands: Optional[bool] = None, modulation: Optional[int] = None, n_fft: int = 64,
           ecc: int = ECC_NONE, fcs: bool = False, scale: float = SC16_DEFAULT_SCALE, **sync) -> bytes:
    """`ofdm::decode!(samples, guard_bands, modulation)` (src/receiver.rs:8-96): Vec<Complex64> -> Result<Vec<u8>>.
    Raises DecodeError("Input not long enough, bailing early") where the reference returns Err.  fcs: the frame was sent with
    encode(..., fcs=True): exactly the payload comes back, or DecodeError when the check fails.  An int16 array of shape [n, 2] is an
    sc16 capture (EXT-9), widened with `scale` on the device."""
    ctx = _ctx(n_fft, BPSK if modulation is None else modulation, bool(guard_bands), _with_fcs(ecc, fcs), **sync)
    arr = np.asarray(samples)
    sc16 = arr.dtype == np.int16
    x = ctx.to_device(_sc16_host(arr, "decode")).unsqueeze(0) if sc16 else ctx.to_device(arr).reshape(1, -1)
    max_symbols = max((x.shape[1] + ctx.S - 1) // ctx.S - 10, 1)
    res = ctx.decode_batch_sc16(x, max_symbols=max_symbols, scale=scale) if sc16 else ctx.decode_batch(x, max_symbols=max_symbols)
    ctx.synchronize()
    status = int(res["status"][0])
    if status == FRAME_SHORT:
        raise DecodeError("Input not long enough, bailing early")
    if status != FRAME_OK:
        raise DecodeError(_FRAME_ERRORS.get(status, "decode failed"))
    n = int(res["len"][0])
    return bytes(res["bytes"][0, :n].cpu().numpy())


def decode_long(samples, guard_bands: Optional[bool] = None, modulation: Optional[int] = None, n_fft: int = 64,
                ecc: int = ECC_NONE, world: int = 1, max_symbols: Optional[int] = None, device: int = 0, fcs: bool = False,
                scale: float = SC16_DEFAULT_SCALE, **sync):
    """`ofdm::decode!` of ONE long capture (the 2 M-sample buffers of examples/jetson_rx.rs:15-17,48-49,84-86) on the HIP path.
    world > 1 rehearses the multi-GPU halo split on one device: `world` contexts, context r searching the lags
    dist.lag_ranges(...)[r] of the shared capture (ofdm_sc_correlate_long), the lowest range with a detection wins
    (dist.merge_first_detection), and that context runs the receive chain (ofdm_rx_decode_long with the merged detection).
    Returns dict(bytes, len, status, offset, f_delta, metric); raises DecodeError where the reference returns Err, and, with fcs (the
    frame was sent with encode(..., fcs=True)), when the frame check fails.  An int16 array of shape [n, 2] is an sc16 capture (EXT-10),
    widened with `scale` on the device (ofdm_rx_decode_long_sc16; world = 1 only)."""
    from . import dist

    mod = BPSK if modulation is None else modulation
    ecc = _with_fcs(ecc, fcs)
    ctxs = [_ctx(n_fft, mod, bool(guard_bands), ecc, device=device, _replica=r, **sync) for r in range(max(world, 1))]
    c0 = ctxs[0]
    sc16 = samples.dtype == torch.int16 if isinstance(samples, torch.Tensor) else np.asarray(samples).dtype == np.int16
    if sc16:
        if world > 1:
            raise OfdmError("decode_long: an sc16 capture is decoded by one context (world = 1)")
        x = samples if isinstance(samples, torch.Tensor) else c0.to_device(_sc16_host(samples, "decode_long"))
        if max_symbols is None:
            max_symbols = max((x.shape[-2] + c0.S - 1) // c0.S - 10, 1)
        return _long_result(c0.decode_long_sc16(x, max_symbols, scale=scale), fcs)
    x = samples if isinstance(samples, torch.Tensor) else c0.to_device(np.asarray(samples))
    x = x.reshape(-1)
    if max_symbols is None:
        max_symbols = max((x.numel() + c0.S - 1) // c0.S - 10, 1)
    if world <= 1 or c0.params.sync_mode != SYNC_SCHMIDL_COX:
        res = c0.decode_long(x, max_symbols)
    else:
        L, W = c0.S, c0.params.sync_window_reps * c0.S
        dets = []
        for (lo, hi), c in zip(dist.lag_ranges(x.numel(), world, L, W), ctxs):
            d, fd, m = c.sc_correlate_long(x, lo, hi) if hi > lo else (-1, 0.0, 0.0)
            dets.append((0, hi, d, fd, m))  # d is already a lag of the whole capture
        d, fd, m = dist.merge_first_detection(dets)
        winner = next((c for c, det in zip(ctxs, dets) if det[2] >= 0), c0)
        res = winner.decode_long(x, max_symbols, d_hat_known=d) if d >= 0 else {
            "bytes": c0.empty((4,), torch.uint8), "len": 0, "status": FRAME_NOSYNC, "offset": 0, "f_delta": 0.0, "metric": 0.0}
    return _long_result(res, fcs)


def decode_all(samples, guard_bands: Optional[bool] = None, modulation: Optional[int] = None, n_fft: int = 64, ecc: int = ECC_NONE,
               fcs: bool = False, holdoff: Optional[int] = None, max_packets: int = 4096, max_symbols: Optional[int] = None,
               lag_lo: int = 0, lag_hi: int = 0, device: int = 0, batched: bool = False, dc_blocks: int = 0, ddc=None, **sync) -> list:
    """EVERY packet of one long capture (EXT-12): one scan for all detections (Context.sc_scan_long: three launches, one
    synchronisation), then decode_long(lag_lo = where the search for packet k started) per detection.  -> a list of per-packet dicts
    (bytes: the payload as `bytes`, empty unless status == FRAME_OK; len, status, offset into the capture, f_delta, metric, d1, d_hat),
    in the order of the capture.  Nothing is raised for a packet that fails: its status is in its dict.

    holdoff: samples from one packet's first threshold crossing to where the search for the next one starts.  None = the shortest
    frame, 11 S - W (at least 1): safe for any traffic, but inside a longer frame's payload the metric may cross the threshold again, and
    every such crossing comes back as a packet of its own (status FRAME_HEADER / FRAME_FCS in the framed, LDPC and frame-check modes;
    with ECC_NONE nothing tells it from a packet).  With frames of ONE size pass the real one: ctx.frame_samples(payload_bytes) - W, or a
    little less.  max_symbols: the data symbols of the longest frame expected (None: up to the capture's end, which costs a demod of
    everything behind every packet).  max_packets stops the scan; a capture with more is cut there (the last dict carries more=True).

    batched=True (EXT-13): the same list from one scan and ONE batched decode (Context.decode_packets) instead of a decode_long per
    packet.  Its f_delta is the scan's own (within 1e-9 of the default path's, whose slice search sums in another order) and its metric
    within 1e-6; every other field is equal.  It requires max_symbols (OfdmError without it: the default "up to the capture's end" would
    gather the capture once per packet).

    dc_blocks (EXT-15, 0 = off): the capture goes through the DC blocker on the device first (Context.dc_block) -- for captures of a
    direct-conversion radio, whose LO leakage fires the detector on noise; frames need guard bands (the DC bin then carries nothing).

    ddc (EXT-16, None = off): (decim, f0, taps) -- the capture is input-rate samples with the signal at f0 cycles per sample; it goes
    through the down-converter on the device first (Context.ddc_once; taps None: ddc_design(decim)), in front of the DC blocker, and
    every offset and lag is in OUTPUT samples."""
    if batched and max_symbols is None:
        raise OfdmError("decode_all(batched=True) requires max_symbols: the data symbols of the longest frame expected")
    ctx = _ctx(n_fft, BPSK if modulation is None else modulation, bool(guard_bands), _with_fcs(ecc, fcs), device=device, **sync)
    x = samples if isinstance(samples, torch.Tensor) else ctx.to_device(np.asarray(samples))
    x = x.reshape(-1)
    if ddc is not None:
        decim, f0, taps = (tuple(ddc) + (None, None))[:3]
        x = ctx.ddc_once(x, decim, ddc_inc_for(f0 or 0.0), taps)
    if dc_blocks:
        x = ctx.dc_block(x, dc_blocks)
    if holdoff is None:
        holdoff = ctx.default_holdoff()
    if max_symbols is None:
        max_symbols = max((x.numel() + ctx.S - 1) // ctx.S - 10, 1)
    det = ctx.sc_scan_long(x, holdoff, max_packets, lag_lo, lag_hi)
    out = []
    if batched:
        res = ctx.decode_packets(x, det, max_symbols)
        ctx.synchronize()
        rows = res["bytes"].cpu().numpy()
        col = {k: res[k].cpu().numpy() for k in ("len", "status", "offset", "f_delta", "metric")}
        for k in range(det["d_hat"].size):
            ok = int(col["status"][k]) == FRAME_OK
            out.append({"bytes": bytes(rows[k, : int(col["len"][k])]) if ok else b"", "len": int(col["len"][k]), "status": int(col["status"][k]),
                        "offset": int(col["offset"][k]), "f_delta": float(col["f_delta"][k]), "metric": float(col["metric"][k]),
                        "d1": int(det["d1"][k]), "d_hat": int(det["d_hat"][k]), "more": False})
        if out and det["more"]:
            out[-1]["more"] = True
        return out
    for k in range(det["d_hat"].size):
        res = ctx.decode_long(x, max_symbols, lag_lo=int(det["lag_lo"][k]), lag_hi=lag_hi)
        ok = res["status"] == FRAME_OK
        res["bytes"] = bytes(res["bytes"][: res["len"]].cpu().numpy()) if ok else b""
        res.update(d1=int(det["d1"][k]), d_hat=int(det["d_hat"][k]), more=False)
        out.append(res)
    if out and det["more"]:
        out[-1]["more"] = True
    return out


def _long_result(res: dict, fcs: bool) -> dict:
    """decode_long's result, or the DecodeError the reference's Err stands for"""
    if res["status"] == FRAME_SHORT:
        raise DecodeError("Input not long enough, bailing early")
    if fcs and res["status"] == FRAME_FCS:
        raise DecodeError(_FRAME_ERRORS[FRAME_FCS])
    return res
