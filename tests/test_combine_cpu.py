"""CPU checks of EXT-7, soft combining: the properties of the definition (tests/combine_ref.py), the merged status / live-symbol rule
of the chain, and the link experiment that shows why the weights come from link quality -- the f64 oracle's frames through two
channels 5 dB apart, LLRs, LLR units and verdicts from the numpy definitions of the stages.  No kernel is launched here; the kernel
is held to combine_ref bit for bit in tests/test_gpu_combine.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import combine_ref as cb  # noqa: E402
import ldpc_ref  # noqa: E402
import quality_ref  # noqa: E402
import soft_ref  # noqa: E402


def _quality(u, valid=None):
    u = np.asarray(u, np.float32)
    q = np.zeros((u.size, cb.QUALITY_FIELDS), np.float32)
    q[:, cb.Q_VALID] = 1.0 if valid is None else valid
    q[:, cb.Q_LLR_UNIT] = u
    return q


def _rows(rng, rows, n_llr):
    return rng.integers(-128, 128, (rows, n_llr)).astype(np.int8)


# ---------------------------------------------------------------------------------------------------------- the definition's properties
def test_one_branch_is_the_identity():
    llr = np.arange(-128, 128).astype(np.int8).reshape(1, -1)
    for quality in (None, _quality([3.5])):
        out, q = cb.combine(llr, 1, quality)
        assert list(q) == [64]
        assert np.array_equal(out[0, 1:], llr[0, 1:]) and out[0, 0] == -127       # -128 becomes -127, everything else itself


@pytest.mark.parametrize("R", [2, 3, 5, 8])
def test_branch_order_does_not_matter(R):
    rng = np.random.default_rng(R)
    F, n = 6, 97
    llr = _rows(rng, F * R, n).reshape(F, R, n)
    u = rng.random((F, R)).astype(np.float32) * 10 + 0.01
    st = (rng.random((F, R)) < 0.2).astype(np.int32) * -2
    nl = rng.integers(-3, n + 5, (F, R)).astype(np.int32)
    out, q = cb.combine(llr.reshape(F * R, n), R, _quality(u.reshape(-1)), st.reshape(-1), nl.reshape(-1))
    perm = rng.permutation(R)
    out2, q2 = cb.combine(llr[:, perm].reshape(F * R, n), R, _quality(u[:, perm].reshape(-1)), st[:, perm].reshape(-1), nl[:, perm].reshape(-1))
    assert np.array_equal(out, out2) and np.array_equal(q.reshape(F, R)[:, perm], q2.reshape(F, R))


def test_a_dead_branch_changes_nothing_whatever_dead_means():
    rng = np.random.default_rng(2)
    n = 64
    live = _rows(rng, 2, n)
    base, qb = cb.combine(live, 2, _quality([2.0, 0.7]))
    assert list(qb) == [64, 22]                                                  # rint(64 * 0.35) = rint(22.4)
    extra = _rows(rng, 1, n)
    three = np.concatenate([live[:1], extra, live[1:]])
    with np.errstate(all="ignore"):
        for status, valid, u in ((-2, 1, 9.0), (0, 0, 9.0), (0, 1, np.nan), (0, 1, np.inf), (0, 1, 0.0), (0, 1, -1.0), (0, 1, -np.inf)):
            out, q = cb.combine(three, 3, _quality([2.0, u, 0.7], [1, valid, 1]), np.array([0, status, 0], np.int32))
            assert np.array_equal(out, base) and list(q) == [64, 0, 22], (status, valid, u)
    # every branch dead: zeros and zero weights
    out, q = cb.combine(three, 3, _quality([2.0, 1.0, 0.7]), np.array([-1, -2, -3], np.int32))
    assert not out.any() and not q.any()


def test_the_best_branch_weighs_64_and_far_branches_drop_out():
    rng = np.random.default_rng(3)
    u = (rng.random((50, 4)) * 100 + 1e-3).astype(np.float32)
    q = cb.weights(50, 4, _quality(u.reshape(-1))).reshape(50, 4)
    assert np.all(q.max(axis=1) == 64) and np.all(q[np.arange(50), u.argmax(axis=1)] == 64) and q.min() >= 0
    # 2^-7 of the best still weighs 64 / 128 = 0.5 -> ties to even = 0; 1.5 / 128 of it weighs 0.75 -> 1; 2^-20 -> 0
    assert list(cb.weights(1, 4, _quality([128.0, 1.0, 1.5, 128.0 * 2.0 ** -20]))) == [64, 0, 1, 0]
    # equal units: an equal-weight sum, as without quality rows
    llr = _rows(rng, 4, 33)
    a, qa = cb.combine(llr, 4, _quality([0.3] * 4))
    b, qb2 = cb.combine(llr, 4)
    assert np.array_equal(a, b) and list(qa) == list(qb2) == [64] * 4


def test_ties_round_to_even():
    for k in range(0, 64):
        q = cb.weights(1, 2, _quality([128.0, 2.0 * k + 1.0]))                  # 64 u / u_max = k + 0.5 exactly
        assert list(q) == [64, k if k % 2 == 0 else k + 1], k


def test_counted_lengths_and_the_rounding_of_the_sum():
    llr = np.array([[100, 100, 100, 100], [-100, -100, -100, -100], [1, -1, 127, -128]], np.int8)
    out, q = cb.combine(llr, 3, None, None, np.array([2, 9, -4], np.int32))     # n_r = 2, 4 (clamped), 0 (clamped)
    assert list(q) == [64, 64, 64] and list(out[0]) == [0, 0, -100, -100]
    out, _ = cb.combine(llr, 3)
    assert list(out[0]) == [1, -1, 127, -127]                                    # 127 and -128 clamp; the shift is a floor after + 32
    # (sum + 32) >> 6 with q = (64, 1): 64 a + b + 32 floors to a for b in [-32, 31]
    two = np.array([[5, 5, -5, -5], [31, 32, -32, -33]], np.int8)
    out, q = cb.combine(two, 2, _quality([64.0, 1.0]))
    assert list(q) == [64, 1] and list(out[0]) == [5, 6, -5, -6]


# ---------------------------------------------------------------------------------------------------------- the chain's merged verdict
def test_merged_status_and_live_symbols_case_by_case():
    R = 3
    ok = _quality([1.0, 2.0, 3.0])
    cases = [  # status_r, nsym_r, quality, want (status_f, nsym_f)
        ([0, 0, 0], [5, 3, 4], ok, (0, 5)),
        ([-2, 0, -1], [0, 3, 0], ok, (0, 3)),                                    # one live branch is enough
        ([-2, -1, -3], [0, 0, 0], ok, (-2, 0)),                                  # none live: the first non-zero status in branch order
        ([0, -3, -1], [5, 0, 0], _quality([1.0, 2.0, 3.0], [0, 1, 1]), (-3, 0)),  # branch 0 has status 0 but no valid quality row
        ([0, 0, 0], [5, 5, 5], _quality([1.0, 2.0, 3.0], [0, 0, 0]), (cb.HEADER_STATUS, 0)),  # every status 0, nothing live
        ([0, 0, 0], [5, 4, 2], _quality([np.nan, 0.0, 3.0]), (0, 2)),            # the live branch's count, not the largest
        ([0, 0, 0], [2, 5, 3], _quality([1.0, 1e-9, 1.0]), (0, 5)),              # a live branch of weight 0 still counts for nsym
    ]
    for st, ns, q, want in cases:
        with np.errstate(all="ignore"):
            got = cb.merge(R, np.array(st, np.int32), np.array(ns, np.int32), q)
        assert (int(got[0][0]), int(got[1][0])) == want, (st, ns)
    # frames side by side
    st = np.array([c[0] for c in cases[:3]], np.int32).reshape(-1)
    ns = np.array([c[1] for c in cases[:3]], np.int32).reshape(-1)
    sf, nf = cb.merge(R, st, ns, np.concatenate([ok] * 3))
    assert list(sf) == [0, 0, -2] and list(nf) == [5, 3, 0]


# ---------------------------------------------------------------------------------------------------------- the link experiment
def test_weighted_combining_beats_the_better_branch_and_the_equal_weight_sum(orc):
    """N = 64, 64-QAM, guard bands, LDPC648, payload 72 bytes (two code words, five data symbols), 100 frames; branch 1 is 5 dB below
    branch 0 (8 dB).  Frames delivered right: weighted combining > branch 0 alone > the equal-weight sum (on the definitions 91 > 82 >
    44): an unweighted sum of a good and a poor capture is WORSE than the good one alone."""
    n, guard, mod, D, frames, s = 64, True, 6, 5, 100, 8.0
    S, cp = 80, 16
    trn = orc.default_training(n)
    bins = soft_ref.data_bins(orc, n, guard)
    nd = bins.size
    body = D * nd * mod // 8 - 16
    rng = np.random.default_rng(5)
    right = {"branch0": 0, "branch1": 0, "weighted": 0, "equal": 0}
    for f in range(frames):
        pay = bytes(rng.integers(0, 256, 72, dtype=np.uint8))
        tx = orc.encode(bytes(ldpc_ref.stream(pay)), True, mod, n)
        L = np.zeros((2, D * nd * mod), np.int8)
        Q = np.zeros((2, cb.QUALITY_FIELDS), np.float32)
        status = np.zeros(2, np.int32)
        for r in range(2):
            y, _ = orc.channel(tx, snr_db=s - 5 * r, timing_error=False, seed=100000 + 2 * f + r)
            rx = np.concatenate([np.zeros(7), y, np.zeros(160)])
            w = orc.decode_sc(rx, guard, mod, n, cfo_off=True, want_soft=True, max_symbols=D)
            status[r] = w["status"]
            if w["status"] != 0 or w["n_symbols"] != D:
                status[r] = status[r] or -1
                continue
            off = w["offset"]
            H = np.fft.fft(rx[off + 5 * S:off + 10 * S].reshape(5, S)[:, cp:].mean(axis=0)) / trn
            L[r] = soft_ref.frame_llrs(w["soft"].reshape(1, D, nd), mod, 32.0, soft_ref.channel_weights(H[None], bins))[0]
            Q[r] = quality_ref.quality(rx[None], n, guard, mod, trn, offset=[off], hk=H)[0]
        verdict = {
            "branch0": L[0] if status[0] == 0 else None, "branch1": L[1] if status[1] == 0 else None,
            "weighted": cb.combine(L, 2, Q, status)[0][0], "equal": cb.combine(L, 2, None, status)[0][0],
        }
        for name, row in verdict.items():
            if row is not None and (status == 0).any():
                st, got = ldpc_ref.receive(row[128:], body)
                right[name] += int(st == 0 and got == pay)
    print(f"frames right of {frames} at {s} dB / {s - 5} dB: {right}")
    assert right["weighted"] > right["branch0"] > right["equal"], right
