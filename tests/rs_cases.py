"""RS(255,223) blocks whose answer is known from how they were built, and the contract check that judges a decoder by them
(tests/test_rs_contract_cpu.py on the host decoder, tests/test_gpu_rs_contract.py on k_rs255_decode).  numpy only.

The contract (README, ofdm_amd/csrc/outer_code.hip): a block decodes to the unique code word within 16 byte errors or fails, a
function of the input alone.  No decoder is needed to check it: with at most 16 injected errors the sent block is the answer (the
minimum distance is 33, so no other code word lies within 16), and whatever is delivered beyond 16 can be re-encoded and counted
against the input.  The encoder below is the instrument that judges the decoder, so GF(2^8) is restated here on its own -- polynomial
0x11d, generator prod_{i<32} (x - 2^i), systematic encoding by synthetic division, byte 0 the highest-degree coefficient -- and
nothing is imported from the library; test_rs_contract_cpu.py holds it to ofdm_rs255_encode."""
import functools

import numpy as np

N, K, PAR, T = 255, 223, 32, 16
SEED = 22333
IS_COUNTS = {"A": 765, "B": 480, "C": 24, "E": 17}         # the blocks judged by "is"; never by the lenient rule
D_WEIGHTS, D_PER_WEIGHT, D_RANDOM = range(17, 41), 32, 256
COUNTS = dict(IS_COUNTS, D=len(D_WEIGHTS) * D_PER_WEIGHT + D_RANDOM)


# ---------------------------------------------------------------------------------------------------------- GF(2^8)
def _tables():
    exp, log = np.zeros(512, np.int64), np.zeros(256, np.int64)
    x = 1
    for i in range(255):
        exp[i], log[x] = x, i
        x <<= 1
        if x & 0x100:
            x ^= 0x11d
    exp[255:510] = exp[:255]
    return exp, log


EXP, LOG = _tables()


def gf_mul(a, b):
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    return np.where((a != 0) & (b != 0), EXP[LOG[a] + LOG[b]], 0)


def _generator():
    g = np.array([1], np.int64)                             # highest degree first
    for i in range(PAR):                                    # g *= (x - 2^i)
        g = np.concatenate([g, [0]]) ^ np.concatenate([[0], gf_mul(g, EXP[i])])
    return g


GEN = _generator()                                          # 33 coefficients, GEN[0] = 1


def encode(data) -> np.ndarray:
    """data [..., 223] -> code words [..., 255]: the data, then the remainder of data(x) x^32 by the monic generator; all rows at once"""
    data = np.asarray(data, np.uint8)
    d = data.reshape(-1, K).astype(np.int64)
    rem = np.zeros((d.shape[0], PAR), np.int64)
    for i in range(K):
        c = d[:, i] ^ rem[:, 0]
        rem = np.concatenate([rem[:, 1:], np.zeros((d.shape[0], 1), np.int64)], axis=1) ^ gf_mul(GEN[None, 1:], c[:, None])
    return np.concatenate([d, rem], axis=1).astype(np.uint8).reshape(data.shape[:-1] + (N,))


# ---------------------------------------------------------------------------------------------------------- the blocks
def _nonzero(rng, n):
    return rng.integers(1, 256, n, dtype=np.uint8)


def _positions_b(rng, kind, w):
    if kind == 1:
        return np.arange(w)
    if kind == 2:
        return np.arange(N - w, N)
    if kind == 3:                                           # a burst with bytes on both sides of a lane boundary
        edge = int(rng.choice([64, 128, 192]))
        return np.arange(w) + edge - int(rng.integers(1, w))
    if kind == 4:
        return K + rng.choice(PAR, w, replace=False)
    if kind == 5:                                           # lanes of k_rs255_decode: one lane holds positions l, l + 64, l + 128, l + 192
        lanes = rng.choice(63, -(-w // 4), replace=False)
        return (lanes[:, None] + 64 * np.arange(4)[None, :]).reshape(-1)[:w]
    return rng.choice(N, w, replace=False)


def _values_b(rng, kind, w):
    if kind == 6:
        return np.full(w, _nonzero(rng, 1)[0], np.uint8)
    if kind == 7:                                           # xor of the values 0: S_0 = 0, the first discrepancy is zero with L = 0
        while True:
            v = _nonzero(rng, w)
            v[-1] = np.bitwise_xor.reduce(v[:-1])
            if v[-1]:
                return v
    return _nonzero(rng, w)


@functools.lru_cache(maxsize=None)
def cases(seed: int = SEED):
    """[(family, received block uint8[255], expectation)], expectation ("is", data bytes, fixed) or ("either",).  One seed, one list;
    the arrays are shared between the tests and must not be written to."""
    rng = np.random.default_rng(seed)
    out = []

    def add(family, block, expectation):
        block = np.ascontiguousarray(block, np.uint8)
        block.setflags(write=False)
        out.append((family, block, expectation))

    n_words = 1 + 32 * (T - 1) + 12 + len(D_WEIGHTS) * D_PER_WEIGHT + 16
    words = iter(encode(rng.integers(0, 256, (n_words, K), dtype=np.uint8)))    # all code words in one go: the encoder is vectorised

    def word():
        return next(words).copy()

    # A: one code word, a single error at every position with each of three values
    c = word()
    for pos in range(N):
        for v in (0x01, 0x80, 0xFF):
            r = c.copy()
            r[pos] ^= v
            add("A", r, ("is", bytes(c[:K]), 1))
    # B: every weight 2 .. 16, 32 blocks each, the eight kinds in turn
    for w in range(2, T + 1):
        for i in range(32):
            kind = i % 8 + 1
            c = word()
            pos, val = _positions_b(rng, kind, w), _values_b(rng, kind, w)
            assert len(set(pos.tolist())) == w and pos.min() >= 0 and pos.max() < N and val.all()
            r = c.copy()
            r[pos] ^= val
            add("B", r, ("is", bytes(c[:K]), w))
    # C: the nearest other code word.  The code word of the data e_222 is the generator polynomial (weight 33); the code is cyclic
    g_word = np.zeros(N, np.int64)
    g_word[K - 1:] = GEN
    for s in (0, 1, 100, 222):
        for a in (0x01, 0x53, 0xFF):
            h = gf_mul(np.roll(g_word, -s), a).astype(np.uint8)
            c = word()
            c2 = c ^ h
            at = np.flatnonzero(h)
            assert at.size == 33
            for j, answer in ((16, c), (17, c2)):           # 16 from c and 17 from c2; 17 from c and 16 from c2
                r = c.copy()
                r[at[:j]] = c2[at[:j]]
                add("C", r, ("is", bytes(answer[:K]), 16))
    # D: beyond capacity
    for w in D_WEIGHTS:
        for _ in range(D_PER_WEIGHT):
            r = word()
            r[rng.choice(N, w, replace=False)] ^= _nonzero(rng, w)
            add("D", r, ("either",))
    for _ in range(D_RANDOM):
        add("D", rng.integers(0, 256, N, dtype=np.uint8), ("either",))
    # E: no errors
    add("E", np.zeros(N, np.uint8), ("is", bytes(K), 0))
    for _ in range(16):
        c = word()
        add("E", c, ("is", bytes(c[:K]), 0))
    assert next(words, None) is None
    return tuple(out)


def family_counts(cs) -> dict:
    n = {}
    for family, _, _ in cs:
        n[family] = n.get(family, 0) + 1
    return n


# ---------------------------------------------------------------------------------------------------------- the contract
def check(block, delivered, fixed, expectation) -> str:
    """Judges what a decoder made of one received block: `delivered` its 223 bytes, `fixed` its corrected count (-1: failed, the
    received data bytes delivered unchanged).  -> "is", "failed" or "decoded"; AssertionError where the contract is broken."""
    block = np.asarray(block, np.uint8)
    delivered, fixed = bytes(delivered), int(fixed)
    assert len(delivered) == K
    if expectation[0] == "is":
        _, data, count = expectation
        assert fixed == count, ("corrected count", fixed, count)
        assert delivered == data, ("bytes", int((np.frombuffer(delivered, np.uint8) != np.frombuffer(data, np.uint8)).sum()))
        return "is"
    assert expectation == ("either",)
    if fixed == -1:
        assert delivered == bytes(block[:K]), "a failed block delivers the received data bytes unchanged"
        return "failed"
    assert 1 <= fixed <= T, ("corrected count", fixed)
    distance = int((encode(np.frombuffer(delivered, np.uint8)) != block).sum())
    assert distance == fixed, ("the delivered code word's distance from the input", distance, fixed)
    return "decoded"


def distances(blocks, delivered) -> np.ndarray:
    """per block, the bytes in which the code word of its 223 delivered bytes differs from the received block (one vectorised encode)"""
    return (encode(np.asarray(delivered, np.uint8)) != np.asarray(blocks, np.uint8)).sum(axis=-1)


def check_uncounted(block, delivered, expectation, distance=None) -> int:
    """check() where the decoder reports no count for the block (a block inside a row of several): the count follows from the bytes.
    A block has "failed" where its data bytes are unchanged and do not belong to a code word within 16 of it -- the contract's first
    arm; a code word within 16 is the only one, so its distance (`distance`: distances() of this block, if the caller has it) is the
    count.  -> the block's corrected count, -1 if it failed"""
    block, delivered = np.asarray(block, np.uint8), bytes(delivered)
    if expectation[0] == "is":
        check(block, delivered, expectation[2], expectation)
        return expectation[2]
    if distance is None:
        distance = int(distances(block, np.frombuffer(delivered, np.uint8)))
    fixed = int(distance) if 1 <= distance <= T else -1
    check(block, delivered, fixed, expectation)
    return fixed


def judge_all(cs, results):
    """check() over the cases and a decoder's [(223 bytes, fixed)] -> {family: {outcome: count}}; asserts the number of "is" blocks"""
    tally = {}
    for i, ((family, block, expectation), (delivered, fixed)) in enumerate(zip(cs, results)):
        try:
            outcome = check(block, delivered, fixed, expectation)
        except AssertionError as e:
            raise AssertionError(f"block {i} of family {family}: {e}") from None
        assert (outcome == "is") == (family != "D"), (i, family, outcome)
        t = tally.setdefault(family, {})
        t[outcome] = t.get(outcome, 0) + 1
    assert len(results) == len(cs)
    assert {f: t.get("is", 0) for f, t in tally.items() if f != "D"} == IS_COUNTS, tally
    return tally
