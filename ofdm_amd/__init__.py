"""ofdm_amd -- MI355X-native OFDM modulate / demodulate hot path (HIP kernels behind a C ABI).

`load()` loads libofdm_hip.so (building it with hipcc when missing) and raises if that fails: there is no
CPU path in this package.  See include/ofdm_hip.h for the boundary and ofdm_amd/api.py for the host mirror
of the reference's function surface.
"""
from ._lib import load, LIB_PATH, Params, SIGNATURES  # noqa: F401


def __getattr__(name):
    # api imports torch and touches the GPU lazily; keep `import ofdm_amd` cheap
    if name in ("api", "Context", "encode", "decode", "decode_long", "decode_all", "pinned_empty", "channel", "default_pilots", "locking_signal", "preamble",
                "training_signals", "OfdmError", "DecodeError", "BPSK", "QPSK", "QAM16", "QAM64", "QAM256",
                "ECC_NONE", "ECC_HAMMING74", "ECC_HAMMING74_SOFT", "ECC_CONV_K7", "ECC_CONV_K7F_R12", "ECC_CONV_K7F_R23", "ECC_CONV_K7F_R34",
                "ECC_RS255", "ECC_RS255_K7F_R12", "ECC_RS255_K7F_R23", "ECC_RS255_K7F_R34", "FRAME_UNCORRECTABLE", "ECC_FCS", "ECC_LDPC648", "ECC_LDPC648_R23", "ECC_LDPC648_R34", "ECC_LDPC648_R56", "LDPC_RATE_1_2", "LDPC_RATE_2_3", "LDPC_RATE_3_4", "LDPC_RATE_5_6", "LDPC_INFO_BYTES", "LDPC_MAX_ITER", "FCS_OVERHEAD", "FRAME_FCS", "crc32",
                "CONV_RATE_1_2", "CONV_RATE_2_3", "CONV_RATE_3_4", "SOFT_LLR_SCALE", "CFO_OFF", "CFO_SIGNED", "CFO_ABS", "CFO_WIDE", "CFO_WIDE_SPAN", "CFO_WIDE_MAX_SPAN", "SYNC_SCHMIDL_COX", "SYNC_REFERENCE",
                "CHEST_LS", "CHEST_WLS", "SC16_DEFAULT_SCALE", "sc16_widen", "sc16_narrow", "Q_VALID", "Q_NOISE_VAR", "Q_GAIN", "Q_SNR", "Q_LLR_UNIT", "Q_EVM2", "Q_POINTS", "QUALITY_FIELDS"):
        import importlib

        api = importlib.import_module(".api", __name__)
        return api if name == "api" else getattr(api, name)
    raise AttributeError(name)
