"""The DC blocker of EXT-15 (include/ofdm_hip.h, "a DC blocker in front of detection") in numpy: THE definition the host functions
ofdm_dc_block / ofdm_dc_block_sc16 and the device handle ofdm_dcblock_* are held to, bit for bit (tests/test_dcblock_cpu.py,
tests/test_gpu_dcblock.py), and a stateful mirror of the handle that shows the rule does not care how a stream is cut.

    blocks of 64 samples, aligned at sample 0; a complete block j has the sum b_j, in f64, by the balanced pairwise tree
    (s = s[0::2] + s[1::2], six times); sample i of block j = i // 64: lo = max(j - M, 0); block 0 passes; otherwise
    acc = b_lo, acc += b_k (k = lo + 1 .. j - 1, ascending), m = acc / (64 (j - lo)), y[i] = x[i] - float32(m), real and imaginary
    part alike and independently.
"""
import numpy as np

BLOCK = 64
MAX_BLOCKS = 1024


def default_blocks(n_fft):
    """ofdm_dc_block_default: ceil(3 S / 64)"""
    S = n_fft + n_fft // 4
    return -(-3 * S // BLOCK)


def widen(q, scale):
    """EXT-9's rule: (float)v * scale, one rounded f32 product per component; q int16 [n, 2] -> complex64 [n]"""
    q = np.asarray(q, np.int16).reshape(-1, 2)
    return np.ascontiguousarray(q.astype(np.float32) * np.float32(scale)).view(np.complex64).reshape(-1)


def block_sums(x):
    """f64 [n // 64, 2]: the pairwise-tree sums of the complete blocks of a complex64 array"""
    x = np.ascontiguousarray(x, np.complex64).reshape(-1)
    nb = x.size // BLOCK
    s = x[: nb * BLOCK].view(np.float32).reshape(nb, BLOCK, 2).astype(np.float64)
    for _ in range(6):
        s = s[:, 0::2] + s[:, 1::2]
    return s.reshape(nb, 2)


def means(b, j_first, j_end, M):
    """float32 [j_end - j_first, 2]: m32 of blocks j_first .. j_end - 1 (j_first >= 1) from the sums b of blocks 0 .. j_end - 2, where
    b[k - base] is the sum of block k: b may hold only the last blocks in front of j_first (base = j_end - 1 - len(b))"""
    j = np.arange(j_first, j_end, dtype=np.int64)
    if j.size == 0:
        return np.zeros((0, 2), np.float32)
    base = j_end - 1 - len(b)
    lo = np.maximum(j - M, 0)
    assert lo.min() >= base and lo.min() >= 0
    with np.errstate(invalid="ignore", over="ignore"):
        acc = b[lo - base].copy()
        for t in range(1, int((j - lo).max())):      # the sequential order: lane = block adds one more block a step
            k = lo + t
            on = k < j
            acc[on] += b[k[on] - base]
        m = acc / (64.0 * (j - lo).astype(np.float64))[:, None]
        return m.astype(np.float32)


def dc_block(x, M):
    """the definition on one whole stream: complex64 [n] -> complex64 [n]"""
    assert 1 <= M <= MAX_BLOCKS
    x = np.ascontiguousarray(x, np.complex64).reshape(-1)
    y = x.copy()
    n_blocks = -(-x.size // BLOCK)
    if n_blocks < 2:
        return y
    m32 = means(block_sums(x)[: n_blocks - 1], 1, n_blocks, M)
    per_sample = np.repeat(m32, BLOCK, axis=0)[: x.size - BLOCK]
    with np.errstate(invalid="ignore", over="ignore"):
        y.view(np.float32).reshape(-1, 2)[BLOCK:] = x.view(np.float32).reshape(-1, 2)[BLOCK:] - per_sample
    return y


def dc_block_sc16(q, scale, M):
    return dc_block(widen(q, scale), M)


class Handle:
    """ofdm_dcblock in numpy: what the device handle carries from push to push -- the sums of the last M complete blocks and the raw
    samples of the open block -- and nothing else"""

    def __init__(self, M):
        assert 1 <= M <= MAX_BLOCKS
        self.M = M
        self.reset()

    def reset(self):
        self.total = 0
        self.sums = np.zeros((0, 2), np.float64)       # blocks total // 64 - len .. total // 64 - 1
        self.open = np.zeros(0, np.complex64)          # total % 64 samples

    def push(self, x):
        x = np.ascontiguousarray(x, np.complex64).reshape(-1)
        if x.size == 0:
            return x.copy()
        j0 = self.total // BLOCK
        z = np.concatenate([self.open, x])             # from sample 64 j0 on
        b = np.concatenate([self.sums, block_sums(z)])  # blocks j0 - len(sums) .. j1 - 1
        j1 = (self.total + x.size) // BLOCK
        j_end = -(-(self.total + x.size) // BLOCK)
        y = z.copy()
        first = max(j0, 1)
        if j_end > first:
            m32 = means(b[: len(b) - (j1 - (j_end - 1))], first, j_end, self.M)
            per = np.repeat(m32, BLOCK, axis=0)[: z.size - (first - j0) * BLOCK]
            with np.errstate(invalid="ignore", over="ignore"):
                y.view(np.float32).reshape(-1, 2)[(first - j0) * BLOCK:] = z.view(np.float32).reshape(-1, 2)[(first - j0) * BLOCK:] - per
        self.sums = b[max(len(b) - self.M, 0):]
        self.open = z[(j1 - j0) * BLOCK:].copy()
        self.total += x.size
        return y[len(z) - x.size:]
