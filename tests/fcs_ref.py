"""The definition of the CRC-32 frame check (include/ofdm_hip.h "frame check sequence", ecc = OFDM_ECC_FCS + mode) in plain Python
over zlib.crc32 -- an implementation of the IEEE 802.3 CRC that shares nothing with the library's.

    envelope   E(payload) = [u32 LE p] ++ payload ++ [u32 LE crc32([u32 LE p] ++ payload)],  p = len(payload)
    check      a delivered row of L bytes is valid iff L >= 8, p = the u32 at byte 0 satisfies p <= L - 8, and the u32 at byte 4 + p
               equals crc32(row[0 : 4 + p]); bytes behind 8 + p are not looked at; a valid row delivers row[4 : 4 + p]
"""
import struct
import zlib

OVERHEAD = 8
ECC_FCS = 64
FRAME_FCS = -6
BASE_MODES = (0, 1, 2, 5, 10, 11, 12, 16, 20, 30, 31, 32, 41, 42, 43)   # every mode the frame check wraps: all of them


def wrap(payload: bytes) -> bytes:
    head = struct.pack("<I", len(payload)) + bytes(payload)
    return head + struct.pack("<I", zlib.crc32(head) & 0xFFFFFFFF)


def check(row: bytes):
    """the payload of a valid row, None for an invalid one"""
    row = bytes(row)
    L = len(row)
    if L < OVERHEAD:
        return None
    p = struct.unpack_from("<I", row, 0)[0]
    if p > L - OVERHEAD:
        return None
    if struct.unpack_from("<I", row, 4 + p)[0] != (zlib.crc32(row[:4 + p]) & 0xFFFFFFFF):
        return None
    return row[4:4 + p]


def clamp(v: int, n: int) -> int:
    return min(max(int(v), 0), n)
