"""GPU checks of EXT-7, soft combining (include/ofdm_hip.h "soft combining"; definition: tests/combine_ref.py):
  1. the stage, ofdm_llr_combine_batch (k_llr_combine), bit for bit against combine_ref over odd sizes, bases and strides, every dead
     case, ties, ragged n_live, guard bytes, and three grids;
  2. the chain with R = 1 against ofdm_rx_decode_batch, bit for bit;
  3. the chain with R = 2 and 3 against the composition of the stage entry points, combine_ref and the modes' CPU frame rules;
  4. argument checks;
  5. weighted combining against the better branch alone and against the equal-weight sum on one link."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import combine_ref as cb  # noqa: E402
import fcs_ref  # noqa: E402
import framed_ref as fr  # noqa: E402
import ldpc_rates_ref as lrr  # noqa: E402
import rs_vectors as rv  # noqa: E402
from chain_checks import KEYS, assert_rows_are, ofdm_api as _api  # noqa: E402
from tools.link import data_snr, link  # noqa: E402

pytestmark = pytest.mark.gpu

N_LLR = (1, 15, 16, 17, 63, 64, 65, 1000, 9792)
FRAMES = (1, 3, 70)
GUARD = 0x55


# ---------------------------------------------------------------------------------------------------------- 1. the stage
def _stage_case(rng, F, R, n_llr):
    """LLRs with -128, and per frame one kind of quality rows: random units, equal units, exact ties (u_max = 128, u = 2 k + 1), ratios
    down to 2^-20, and every way of being dead (status, valid = 0, u NaN / inf / 0 / negative) -- also for every branch of a frame"""
    rows = F * R
    llr = rng.integers(-128, 128, (rows, n_llr)).astype(np.int8)
    llr[rng.random((rows, n_llr)) < 0.05] = -128
    q = np.zeros((rows, cb.QUALITY_FIELDS), np.float32)
    q[:, cb.Q_VALID] = 1.0
    q[:, 1:4] = rng.random((rows, 3))                                            # the other fields are not read
    u = (rng.random((F, R)) * 50 + 0.05).astype(np.float32)
    status = np.zeros((F, R), np.int32)
    valid = np.ones((F, R), np.float32)
    for f in range(F):
        kind = f % 7
        if kind == 1:
            u[f] = 0.37
        elif kind == 2:
            u[f] = 2.0 * rng.integers(0, 64, R) + 1.0
            u[f, rng.integers(0, R)] = 128.0
        elif kind == 3:
            u[f] = 128.0 * 2.0 ** -rng.integers(0, 21, R).astype(np.float64)
            u[f, rng.integers(0, R)] = 128.0
        elif kind == 4:
            for r in range(R):
                how = rng.integers(0, 9)
                if how == 0: status[f, r] = -rng.integers(1, 7)
                elif how == 1: valid[f, r] = 0.0
                elif how in (2, 3, 4, 5, 6): u[f, r] = (np.nan, np.inf, 0.0, -1.5, -np.inf)[how - 2]
        elif kind == 5:                                                          # nothing live at all
            status[f] = -2 if f % 2 else 0
            valid[f] = 0.0
    q[:, cb.Q_VALID] = valid.reshape(-1)
    q[:, cb.Q_LLR_UNIT] = u.reshape(-1)
    n_live = rng.integers(-2, n_llr + 3, rows).astype(np.int32)
    n_live[rng.random(rows) < 0.4] = n_llr                                       # whole branches too: the 16-byte path
    n_live[rng.random(rows) < 0.1] = 0
    n_live[rng.random(rows) < 0.1] = n_llr + 1000
    return llr, q, status.reshape(-1), n_live


def _strided(c, a, base, stride, fill):
    """a [rows, n] int8 on the device as a view with the given byte base and row stride of a buffer filled with `fill`"""
    rows, n = a.shape
    buf = torch.full((base + rows * stride + 64,), fill, dtype=torch.int8, device=c.device)
    view = buf.as_strided((rows, n), (stride, 1), base)
    view.copy_(torch.from_numpy(a).to(c.device))
    return buf, view


@pytest.mark.parametrize("R", [1, 2, 3, 4, 5, 8])
def test_stage_matches_the_definition_bit_for_bit(R):
    api = _api()
    c = api.Context(n_fft=64, modulation=api.QPSK)
    rng = np.random.default_rng(100 + R)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device=c.device, dtype=dt)  # noqa: E731
    paths = set()
    for n_llr in N_LLR:
        for F in FRAMES:
            llr, q, status, n_live = _stage_case(rng, F, R, n_llr)
            with np.errstate(all="ignore"):
                want, wq = cb.combine(llr, R, q, status, n_live)
                plain, pq = cb.combine(llr, R)
            up = (n_llr + 15) // 16 * 16
            for aligned in (True, False):
                base_in, base_out = (0, 0) if aligned else (1, 3)
                s_in = up + 16 if aligned else n_llr + 7 + (n_llr % 2)            # unaligned: an odd stride
                s_out = up + 32 if aligned else n_llr + 9 + (n_llr % 2)
                _, src = _strided(c, llr, base_in, s_in, 0)
                args = (dev(q, torch.float32), dev(status, torch.int32), dev(n_live, torch.int32))
                results = []
                for cap in (0, 1, 3):
                    c.set_tuning("grid_cap", cap)
                    buf, dst = _strided(c, np.zeros((F, n_llr), np.int8), base_out, s_out, GUARD)
                    dst.fill_(GUARD)
                    out, w = c.llr_combine(src, R, *args, out=dst, want_weight=True)
                    c.synchronize()
                    assert out is dst and c.last_dispatch() == "k_llr_combine"
                    host = buf.cpu().numpy()
                    got = np.lib.stride_tricks.as_strided(host[base_out:], (F, n_llr), (s_out, 1))
                    assert np.array_equal(got, want), (n_llr, F, aligned, cap)
                    mask = np.ones(host.size, bool)                              # every byte outside the rows' n_llr is untouched
                    for f in range(F):
                        mask[base_out + f * s_out:base_out + f * s_out + n_llr] = False
                    assert np.all(host[mask] == GUARD), (n_llr, F, aligned, cap)
                    assert np.array_equal(w.cpu().numpy(), wq), (n_llr, F, aligned, cap)
                    results.append(host)
                c.set_tuning("grid_cap", 0)
                assert all(np.array_equal(results[0], r) for r in results[1:])
                # no quality rows, no status, no lengths: the equal-weight sum of every branch
                out, w = c.llr_combine(src, R, want_weight=True)
                assert np.array_equal(out.cpu().numpy(), plain) and np.array_equal(w.cpu().numpy(), pq)
                paths.add(aligned)
    # a 3-D view with one row stride is the same batch
    llr, q, status, n_live = _stage_case(rng, 3, R, 64)
    with np.errstate(all="ignore"):
        want, _ = cb.combine(llr, R, q, status, n_live)
    got = c.llr_combine(dev(llr, torch.int8).view(3, R, 64), R, dev(q, torch.float32), dev(status, torch.int32), dev(n_live, torch.int32))
    assert np.array_equal(got.cpu().numpy(), want) and paths == {True, False}


# ---------------------------------------------------------------------------------------------------------- 2. R = 1 is decode_batch
@pytest.mark.parametrize("n", [64, 128])
@pytest.mark.parametrize("ecc", [16, 41, 42, 43, 10, 11, 12, 80, 30])
def test_one_branch_chain_is_decode_batch(ecc, n):
    api = _api()
    c, pay, rx, D = link(ecc, n, api.QAM64, 8, 300, data_snr(n, 25.0), 40 + ecc)
    g = torch.Generator(device=c.device)
    g.manual_seed(2)
    rx[3] = 1e-3 * torch.randn(rx.shape[1], dtype=torch.complex64, device=c.device, generator=g)     # a slot without a packet
    a = c.decode_batch(rx, max_symbols=D)
    names = c.last_dispatch().split("+")
    b = c.decode_combine(rx.view(8, 1, -1), max_symbols=D)
    c.synchronize()
    trace = c.last_dispatch().split("+")
    assert "k_llr_combine" in trace and "k_linkq" in trace and trace[-1] == names[-1]
    for k in KEYS:
        assert torch.equal(a[k], b[k].view(-1)), k
    assert torch.equal(b["branch_status"].view(-1)[a["status"] == 0], a["status"][a["status"] == 0])
    la = a["len"].cpu().numpy()
    ba, bb = a["bytes"].cpu().numpy(), b["bytes"].cpu().numpy()
    for f in range(8):
        assert bytes(ba[f, :la[f]]) == bytes(bb[f, :la[f]]), f
    status = a["status"].cpu().numpy()
    assert status[3] != 0 and int((status == 0).sum()) >= 5
    assert list(b["weight"].view(-1).cpu().numpy()) == [64 if s == 0 else 0 for s in b["branch_status"].view(-1).cpu().numpy()]


# ---------------------------------------------------------------------------------------------------------- 3. chain = composition
def _branch_captures(c, pay, R, snrs, seed, cut_branch=None):
    """[F, R, span] captures of the frames of pay: branch r through ofdm_channel_batch at snrs[r] with its own seed, delay 1 .. 8 and CFO;
    cut_branch: that branch of every frame arrives 150 samples late, so that a capture length of frame + 48 cuts its last symbols"""
    tx = c.encode_batch(pay)
    F = tx.shape[0]
    g = torch.Generator(device=c.device)
    g.manual_seed(seed)
    rows = []
    for r in range(R):
        d = torch.randint(1, 9, (F,), dtype=torch.int32, device=c.device, generator=g)
        if r == cut_branch:
            d = d + 150
        fd = (torch.rand((F,), dtype=torch.float64, device=c.device, generator=g) - 0.5) * (2.0 / c.S)
        rows.append(c.channel_batch(tx, snr_db=snrs[r], seed=seed + r, delay=d, f_delta=fd, span=tx.shape[1] + 160))
    return torch.stack(rows, dim=1).contiguous()


def _inner_rule(ecc, llr_row, body):
    """(status, bytes) of a combined row by the inner mode's CPU frame rule"""
    if ecc in lrr.ECC:
        return lrr.code_of_ecc(ecc).receive(llr_row[128:], body)
    return fr.decode_stream(llr_row[128:], body, ecc - 10)


def _composition(api, c, c0, rx, D, frame_len):
    """{frame: (status, out_len, bytes)} and the reference's per-branch weights, from the stage entry points, combine_ref and the CPU
    frame rules; the per-branch status, offset and f_delta are decode_batch's on a context without a code"""
    from tools.bench_combine import branch_stages

    F, R, _ = rx.shape
    s = branch_stages(c, c0, rx, D, frame_len=frame_len)
    c.synchronize()
    status, nsym = s["status"].cpu().numpy(), s["nsym"].cpu().numpy()
    quality, L = s["quality"].cpu().numpy(), s["llr"].cpu().numpy()
    with np.errstate(all="ignore"):
        comb, q = cb.combine(L, R, quality, status, s["n_live"].cpu().numpy())
        st_f, nsym_f = cb.merge(R, status, nsym, quality)
    fcs = c.ecc >= api.ECC_FCS
    base = c.ecc - api.ECC_FCS if fcs else c.ecc
    rs = base in (30, 31, 32)
    inner = base - 20 if rs else base
    want = {}
    for f in range(F):
        if st_f[f] != 0:
            want[f] = (int(st_f[f]), 0, b"")
            continue
        st, data = _inner_rule(inner, comb[f], int(nsym_f[f]) * c.bytes_per_symbol - 16)
        if st == 0 and rs:
            out, out_len, fixed = rv.host_row(c.lib, np.frombuffer(data, np.uint8), len(data))
            st, data = (-5, b"") if fixed < 0 else (0, out[:out_len])
        if st == 0 and fcs:
            inside = fcs_ref.check(data)
            st, data = (fcs_ref.FRAME_FCS, b"") if inside is None else (0, inside)
        want[f] = (st, len(data), data)
    return want, q, s


@pytest.mark.parametrize("ecc,R,chest", [(16, 2, 0), (16, 3, 1), (42, 2, 0), (11, 3, 0), (12, 2, 1), (80, 3, 0), (30, 2, 0)])
def test_chain_is_the_composition_of_the_stages(ecc, R, chest):
    api = _api()
    n, mod, F, payload = 64, api.QAM64, 7, 200
    c = api.Context(n_fft=n, modulation=mod, guard_bands=True, ecc=ecc, chest_mode=chest)
    c0 = api.Context(n_fft=n, modulation=mod, guard_bands=True, ecc=api.ECC_NONE, chest_mode=chest)
    g = torch.Generator(device=c.device)
    g.manual_seed(ecc)
    pay = torch.randint(0, 256, (F, payload), dtype=torch.uint8, device=c.device, generator=g)
    D = c.data_symbols(payload)
    rx = _branch_captures(c, pay, R, [20.0 - 4.0 * r for r in range(R)], 900 + ecc, cut_branch=R - 1)
    noise = lambda: 1e-3 * torch.randn(rx.shape[2], dtype=torch.complex64, device=c.device, generator=g)  # noqa: E731
    rx[1, 0] = noise()                                                           # a noise-only branch
    for r in range(R):                                                           # every branch dead
        rx[4, r] = noise()
    frame_len = c.frame_samples(payload) + 48                                    # the late branch is cut inside its data symbols
    results = []
    for chunk in (0, 1, 3):
        c.set_tuning("soft_chunk_frames", chunk)
        res = c.decode_combine(rx, max_symbols=D, frame_len=frame_len)
        c.synchronize()
        trace = c.last_dispatch().split("+")
        assert "k_llr_combine" in trace and "k_linkq" in trace and "k_sym<llr>" in trace and ("k_chest_solve" in trace) == bool(chest)
        results.append(res)
    c.set_tuning("soft_chunk_frames", 0)
    want, q, s = _composition(api, c, c0, rx, D, frame_len)
    res = results[0]
    nsym = s["nsym"].view(F, R).cpu().numpy()
    assert (nsym[:, R - 1] < D).all() and (nsym[[0, 2, 3, 5, 6], 0] == D).all(), nsym    # the cut branch is cut, the others whole
    assert (nsym[:, R - 1] > 0).sum() >= 4
    assert torch.equal(res["branch_status"].view(-1), s["status"]) and torch.equal(res["offset"].view(-1), s["offset"])
    assert torch.equal(res["f_delta"].view(-1), s["f_delta"]) and torch.equal(res["metric"].view(-1), s["metric"])
    assert torch.equal(res["quality"].view(F * R, -1), s["quality"])
    assert np.array_equal(res["weight"].view(-1).cpu().numpy(), q)
    status = res["status"].cpu().numpy()
    bs = res["branch_status"].cpu().numpy()
    assert bs[1, 0] != 0 and (bs[4] != 0).all() and status[4] == bs[4, 0] and status[1] == want[1][0]
    assert_rows_are(res, want)
    good = [f for f, (st, n_out, data) in want.items() if st == 0 and data[:payload] == bytes(pay[f].cpu().numpy())]  # (RS delivers whole blocks)
    print(f"ecc {ecc}, R {R}, chest {chest}: statuses {status.tolist()}, weights {q.reshape(F, R).tolist()}, {len(good)} of {F} whole")
    assert len(good) >= 4
    for other in results[1:]:                                                    # chunks of 1 and 3 frames: the same rows
        assert_rows_are(other, want)
        for k in ("status", "len", "branch_status", "weight", "offset"):
            assert torch.equal(other[k], res[k]), k


# ---------------------------------------------------------------------------------------------------------- 4. arguments
def test_unsupported_modes_and_bad_sizes():
    api = _api()
    for ecc in (0, 1, 2, 5, 20, 64, 64 + 20, 64 + 5):                           # the length header of these comes from one capture's hard bits
        c = api.Context(n_fft=64, modulation=api.QPSK, guard_bands=True, ecc=ecc)
        x = c.to_device(np.ones((2, 2, 2000), np.complex64))
        ob = c.decode_row_bytes(10)
        out = torch.zeros((2, ob), dtype=torch.uint8, device=c.device)
        i32 = torch.zeros((4,), dtype=torch.int32, device=c.device)
        assert c.lib.ofdm_rx_decode_combine_batch(c.h, x.data_ptr(), 2, 2, 2000, 2000, 0, 10, out.data_ptr(), ob, i32.data_ptr(), i32[2:].data_ptr(),
                                                  None, None, None, None, None, None) == -2, ecc
        with pytest.raises(api.OfdmError):
            c.decode_combine(x, max_symbols=10)
    c = api.Context(n_fft=64, modulation=api.QPSK, guard_bands=True, ecc=api.ECC_LDPC648)
    x = c.to_device(np.ones((2, 2, 2000), np.complex64))
    D = 10
    ob = c.decode_row_bytes(D)
    out = torch.zeros((2, ob), dtype=torch.uint8, device=c.device)
    i32 = torch.zeros((4,), dtype=torch.int32, device=c.device)
    f = c.lib.ofdm_rx_decode_combine_batch
    X, O, L, S = x.data_ptr(), out.data_ptr(), i32.data_ptr(), i32[2:].data_ptr()
    tail = (None, None, None, None, None, None)
    assert f(c.h, X, 2, 2, 2000, 2000, 0, D, O, ob, L, S, *tail) == 0
    bad = [f(None, X, 2, 2, 2000, 2000, 0, D, O, ob, L, S, *tail),
           f(c.h, X, 2, 0, 2000, 2000, 0, D, O, ob, L, S, *tail),
           f(c.h, X, 2, 9, 2000, 2000, 0, D, O, ob, L, S, *tail),
           f(c.h, X, -1, 2, 2000, 2000, 0, D, O, ob, L, S, *tail),
           f(c.h, None, 2, 2, 2000, 2000, 0, D, O, ob, L, S, *tail),
           f(c.h, X, 2, 2, 2000, 2000, 0, D, None, ob, L, S, *tail),
           f(c.h, X, 2, 2, 2000, 2000, 0, D, O, ob, None, S, *tail),
           f(c.h, X, 2, 2, 2000, 2000, 0, D, O, ob, L, None, *tail),
           f(c.h, X, 2, 2, 2000, 0, 0, D, O, ob, L, S, *tail),
           f(c.h, X, 2, 2, 2000, 2000, 0, 0, O, ob, L, S, *tail),
           f(c.h, X, 2, 2, 0, 2000, 0, D, O, ob, L, S, *tail),
           f(c.h, X, 2, 2, 2000, 2000, 0, D, O, 31, L, S, *tail)]                # the mode's row for D = 10 is 40 - 8 bytes
    assert ob == 32 and bad == [-1] * len(bad), bad
    assert f(c.h, None, 0, 2, 2000, 2000, 0, D, None, ob, None, None, *tail) == 0
    # the stage
    c.fft(c.to_device(np.ones((1, 64), np.complex64)))
    g = c.lib.ofdm_llr_combine_batch
    llr = torch.zeros((4, 64), dtype=torch.int8, device=c.device)
    dst = torch.full((2, 64), GUARD, dtype=torch.int8, device=c.device)
    A, B = llr.data_ptr(), dst.data_ptr()
    bad = [g(None, A, 2, 2, 64, 64, None, None, None, B, 64, None), g(c.h, None, 2, 2, 64, 64, None, None, None, B, 64, None),
           g(c.h, A, 2, 2, 64, 64, None, None, None, None, 64, None), g(c.h, A, -1, 2, 64, 64, None, None, None, B, 64, None),
           g(c.h, A, 2, 0, 64, 64, None, None, None, B, 64, None), g(c.h, A, 2, 9, 64, 64, None, None, None, B, 64, None),
           g(c.h, A, 2, 2, 63, 64, None, None, None, B, 64, None), g(c.h, A, 2, 2, 64, 64, None, None, None, B, 63, None),
           g(c.h, A, 2, 2, 64, -1, None, None, None, B, 64, None)]
    assert bad == [-1] * len(bad), bad
    assert g(c.h, None, 0, 2, 64, 64, None, None, None, None, 64, None) == 0
    c.synchronize()
    assert c.last_dispatch() == "k_sym<fft>" and bool((dst == GUARD).all())      # nothing was launched, nothing written
    assert g(c.h, A, 2, 2, 64, 64, None, None, None, B, 64, None) == 0 and c.last_dispatch() == "k_llr_combine"
    with pytest.raises(api.OfdmError):
        c.llr_combine(llr, 3)
    with pytest.raises(api.OfdmError):
        c.llr_combine(llr, 2, status=torch.zeros(3, dtype=torch.int32, device=c.device))


# ---------------------------------------------------------------------------------------------------------- 5. it earns its keep
def test_combining_earns_its_keep_on_one_link():
    """256 frames, N = 64, 64-QAM, LDPC648, payload 560, branch 1 5 dB below branch 0, at the point of tools/bench_combine.py's skewed
    sweep at which branch 0 alone delivers nearest to 80 % right (profiles/combine_ber_and_speed.json, block `point`; the link is that
    point's: the same seed and draws).  The ordering is the CPU experiment's (tests/test_combine_cpu.py): weighted combining beats the
    better branch alone, and the equal-weight sum.
    Record (one MI355X): at 4 dB branch 0 alone delivers 194 of 256 right (3 dB: 147, 5 dB: 241), weighted combining 237, the
    equal-weight sum 139, branch 1 alone (at -1 dB) 0."""
    api = _api()
    from tools.bench_combine import PAYLOAD, SKEW_DB, contexts, point_counts, sweep_seed

    snr = POINT_SNR_DB
    c, c0 = contexts()
    row = point_counts(c, c0, [snr, snr - SKEW_DB], 256, sweep_seed(snr), PAYLOAD)
    print(f"{snr} dB / {snr - SKEW_DB} dB, frames right of 256: {({k: v['right'] for k, v in row.items()})}")
    assert api.ECC_LDPC648 == 16
    assert row["weighted"]["right"] > row["branch0"]["right"], row
    assert row["weighted"]["right"] > row["equal_weight"]["right"], row


# the point of the committed record's skewed sweep at which branch 0 alone delivers nearest to 80 % of its frames right
POINT_SNR_DB = 4.0
