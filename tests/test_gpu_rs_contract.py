"""k_rs255_decode held to the RS(255,223) contract by construction: "a block decodes to the unique code word within 16 byte errors
or fails, a function of the input alone".  The blocks of tests/rs_cases.py -- a single error at every position, every weight 2 .. 16
in bursts over the lane boundaries, four roots in one lane, zero first discrepancies, the nearest other code word, 17 .. 40 errors and
noise -- go through Context.rs255_decode one block a row and three blocks a row; what comes back is judged by rs_cases.check (an
encoder, no decoder) and must equal the host decoder of outer_code.hip byte for byte.  Nothing here has a tolerance."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rs_cases as rc  # noqa: E402
import rs_vectors as rv  # noqa: E402
from chain_checks import ofdm_api as _api  # noqa: E402

pytestmark = pytest.mark.gpu

SHUFFLE_SEED = 765


@pytest.fixture(scope="module")
def stage():
    api = _api()
    return api.Context(n_fft=64, modulation=api.QAM64, guard_bands=True, ecc=api.ECC_RS255)


def _strided(c, rows: np.ndarray, slack: int) -> torch.Tensor:
    """the rows on the device with a row stride `slack` bytes larger than the row (0xEE in between), as in tests/test_gpu_rs.py"""
    n, nb = rows.shape
    big = torch.full((n, nb + slack), 0xEE, dtype=torch.uint8, device=c.device)
    big[:, :nb] = torch.from_numpy(np.ascontiguousarray(rows)).to(c.device)
    return big[:, :nb]


def _decode(c, dev):
    got = c.rs255_decode(dev)
    c.synchronize()
    assert "k_rs255_decode" in c.last_dispatch(), c.last_dispatch()
    return tuple(t.cpu().numpy() for t in got)


def _assert_is_the_host_decoder(c, rows, out, out_len, fixed):
    n_code = rows.shape[1]
    for r in range(rows.shape[0]):
        want, want_len, want_fixed = rv.host_row(c.lib, rows[r], n_code)
        assert (int(out_len[r]), int(fixed[r])) == (want_len, want_fixed), (r, out_len[r], fixed[r], want_len, want_fixed)
        assert bytes(out[r]) == want, r


def test_one_block_a_row(stage):
    c = stage
    cs = rc.cases()
    rows = np.array([block for _, block, _ in cs])
    out, out_len, fixed = _decode(c, _strided(c, rows, 7))
    assert out.shape == (len(cs), 2 * rc.K) and (out_len == 2 * rc.K).all()
    assert not out[:, rc.K:].any()                                      # the empty block behind every row
    tally = rc.judge_all(cs, [(bytes(out[r, :rc.K]), int(fixed[r])) for r in range(len(cs))])
    d = tally["D"]
    print(f"family D: {d.get('decoded', 0)} of {sum(d.values())} blocks beyond capacity decoded to another code word (not capped)")
    assert sum(d.values()) == rc.COUNTS["D"]
    _assert_is_the_host_decoder(c, rows, out, out_len, fixed)


def test_three_blocks_a_row(stage):
    c = stage
    cs = rc.cases()
    assert len(cs) % 3 == 0
    order = np.random.default_rng(SHUFFLE_SEED).permutation(len(cs))   # failing blocks between correctable ones
    n_rows = len(cs) // 3
    rows = np.array([cs[i][1] for i in order]).reshape(n_rows, 3 * rc.N)
    dev = _strided(c, rows, 5)
    out, out_len, fixed = _decode(c, dev)
    assert out.shape == (n_rows, 4 * rc.K) and (out_len == 4 * rc.K).all()
    assert not out[:, 3 * rc.K:].any()
    delivered = out[:, :3 * rc.K].reshape(len(cs), rc.K)
    distance = rc.distances(rows.reshape(len(cs), rc.N), delivered)
    judged, mixed = 0, 0
    for r in range(n_rows):
        counts = []
        for b in range(3):
            family, block, expectation = cs[order[3 * r + b]]
            try:
                counts.append(rc.check_uncounted(block, delivered[3 * r + b], expectation, distance[3 * r + b]))
            except AssertionError as e:
                raise AssertionError(f"row {r} block {b} (case {order[3 * r + b]}, family {family}): {e}") from None
            judged += expectation[0] == "is"
        want = -1 if min(counts) < 0 else sum(counts)
        assert int(fixed[r]) == want, (r, counts, int(fixed[r]))
        mixed += min(counts) < 0 <= max(counts)
    assert judged == sum(rc.IS_COUNTS.values()) == 765 + 480 + 24 + 17
    assert mixed >= 100, mixed                                          # rows in which a failing block sits beside correctable ones
    _assert_is_the_host_decoder(c, rows, out, out_len, fixed)
    for cap in (1, 3):                                                  # one workgroup, and a grid that does not divide the rows
        c.set_tuning("grid_cap", cap)
        try:
            again = _decode(c, dev)
        finally:
            c.set_tuning("grid_cap", 0)
        for a, b in zip(again, (out, out_len, fixed)):
            np.testing.assert_array_equal(a, b, err_msg=str(cap))
