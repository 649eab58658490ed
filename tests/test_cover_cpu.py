"""CPU checks of the pairwise cover of the decode chain's options (tests/cover_cases.py; DESIGN.md section 2, "The options meet"):
  1. the committed table is a cover -- computed from the factor lists, not from the generator -- of allowed rows only, at most 100 of
     them, none of which the cover holds without; a table with one pair knocked out is seen;
  2. ofdm_create refuses every excluded pair (and the one excluded triple) and takes every row's options;
  3. receiver_ref.mode_encode has the length chain_refs.mode_coded_len gives, for all 30 modes;
  4. the link: every row has a seed among its eight whose three captures lock on the reference alone (tests/test_gpu_cover.py decodes
     exactly these), and the finding behind the blanked preamble copies of the rows with sync_window_reps < 3."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_refs  # noqa: E402
import cover_cases as cc  # noqa: E402
import receiver_ref as rr  # noqa: E402


# ---------------------------------------------------------------------------------------------------------- 1. the table
def _wanted():
    """the allowed pairs {frozenset of two (factor name, value)}, by brute force: a pair is allowed when some setting of the factors
    the constraints read, the pair's own values fixed, is an allowed row"""
    idx = [cc.NAMES.index(n) for n in cc.CONSTRAINED]
    base = [vals[0] for _, vals in cc.FACTORS]
    want = set()
    for a, b in itertools.combinations(range(len(cc.FACTORS)), 2):
        free = [i for i in idx if i not in (a, b)]
        for v in cc.FACTORS[a][1]:
            for w in cc.FACTORS[b][1]:
                for combo in itertools.product(*[cc.FACTORS[i][1] for i in free]):
                    row = list(base)
                    row[a], row[b] = v, w
                    for i, x in zip(free, combo):
                        row[i] = x
                    if cc.allowed(row):
                        want.add(frozenset(((cc.NAMES[a], v), (cc.NAMES[b], w))))
                        break
    return want


WANTED = _wanted()


def _missing(rows):
    """allowed pairs that no row holds"""
    held = set()
    for row in rows:
        held |= {frozenset(p) for p in itertools.combinations(list(zip(cc.NAMES, row)), 2)}
    return WANTED - held


def test_the_table_is_a_cover():
    assert 0 < len(cc.ROWS) <= 100 and len(set(cc.ROWS)) == len(cc.ROWS)
    for row in cc.ROWS:
        assert len(row) == len(cc.FACTORS) and all(v in vals for v, (_, vals) in zip(row, cc.FACTORS)), row
        assert cc.allowed(row) and cc.carried(row), row
    missing = _missing(cc.ROWS)
    print(f"{len(WANTED)} allowed pairs in {len(cc.ROWS)} rows")
    assert not missing, sorted(map(sorted, missing))[:5]
    # the two ways of counting agree (tools/cover_rows.py uses the second): all 1112 pairs less the 16 excluded ones
    assert len(WANTED) == len(cc.allowed_pairs()) == 1096
    assert {frozenset(((cc.NAMES[i], v), (cc.NAMES[j], w))) for (i, v), (j, w) in cc.allowed_pairs()} == WANTED


def test_every_row_is_needed_and_a_knocked_out_pair_is_seen():
    for i in range(len(cc.ROWS)):
        assert _missing(cc.ROWS[:i] + cc.ROWS[i + 1:]), f"row {i} is redundant: {cc.ROWS[i]}"
    # one pair knocked out: a pair of n_fft and inner mode that one row alone holds gets another inner mode there
    count = {}
    for r in cc.ROWS:
        count[(r[0], r[3])] = count.get((r[0], r[3]), 0) + 1
    n, inner = sorted(p for p, c in count.items() if c == 1)[0]
    hit = next(i for i, r in enumerate(cc.ROWS) if (r[0], r[3]) == (n, inner))
    other = next(r[3] for r in cc.ROWS if r[0] == n and r[3] != inner and cc.allowed(cc.ROWS[hit][:3] + (r[3],) + cc.ROWS[hit][4:]))
    rows = list(cc.ROWS)
    rows[hit] = rows[hit][:3] + (other,) + rows[hit][4:]
    assert frozenset((("n_fft", n), ("inner", inner))) in _missing(rows)


def test_the_excluded_pairs_are_the_constraints():
    bad = {frozenset(p) for p in cc.excluded_pairs()}
    rs = {frozenset((("inner", i), ("outer", o))) for i in (1, 2, 5, 16, 41, 42, 43) for o in (cc.OUTER_RS, cc.OUTER_BOTH)}
    assert bad == rs | {frozenset((("sync_mode", cc.REFERENCE), ("cfo_mode", cc.CFO_WIDE))),
                        frozenset((("cfo_mode", cc.CFO_WIDE), ("sync_backoff", cc.BACKOFF_CP)))}
    every = {frozenset(((a, v), (b, w))) for (a, va), (b, vb) in itertools.combinations(cc.FACTORS, 2) for v in va for w in vb}
    assert len(every) == 1112 and every - bad == WANTED
    # the third constraint also rules out a triple no pair shows: WLS with a back-off of cp_len is allowed under SYNC_REFERENCE only
    row = dict(zip(cc.NAMES, [vals[0] for _, vals in cc.FACTORS]), chest_mode=cc.WLS, sync_backoff=cc.BACKOFF_CP)
    assert not cc.allowed(tuple(row.values())) and cc.allowed(tuple({**row, "sync_mode": cc.REFERENCE}.values()))


# ---------------------------------------------------------------------------------------------------------- 2. the library's constraints
@pytest.fixture(scope="module")
def lib():
    from ofdm_amd import build

    return C.CDLL(build.build())


def _create(lib, k=None, **over):
    from ofdm_amd import Params

    p = Params()
    lib.ofdm_default_params(C.byref(p))
    if k is not None:
        kw = k.context_kw()
        p.n_fft, p.cp_len, p.modulation, p.guard_bands, p.ecc = kw["n_fft"], kw["n_fft"] // 4, kw["modulation"], int(kw["guard_bands"]), kw["ecc"]
        p.sync_window_reps, p.sync_backoff, p.cfo_mode, p.sync_threshold = kw["sync_window_reps"], kw["sync_backoff"], kw["cfo_mode"], kw["sync_threshold"]
        p.sync_mode, p.chest_mode = kw["sync_mode"], kw["chest_mode"]
    for name, v in over.items():
        setattr(p, name, v)
    h = C.c_void_p()
    rc = lib.ofdm_create(C.byref(p), None, None, 0, None, C.byref(h))
    if rc == 0:
        lib.ofdm_destroy(h)
    return rc


def _params_of(pair):
    """an excluded pair as fields of ofdm_params (n_fft 64: cp_len 16)"""
    d = dict(pair)
    kw = {name: d[name] for name in ("sync_mode", "cfo_mode", "chest_mode") if name in d}
    if "inner" in d or "outer" in d:
        kw["ecc"] = d.get("inner", 0) + d.get("outer", 0)
    if "sync_backoff" in d:
        kw["sync_backoff"] = 16 if d["sync_backoff"] == cc.BACKOFF_CP else d["sync_backoff"]
    return kw


def test_create_refuses_every_excluded_pair_and_takes_every_row(lib):
    import torch

    want = 0 if torch.cuda.is_available() else -3          # OFDM_ERR_NO_DEVICE without a GPU, as for any valid set of options
    for pair in cc.excluded_pairs():
        kw = _params_of(pair)
        assert _create(lib, **kw) == -1, pair
        for name, v in kw.items():                         # each half alone is taken
            assert _create(lib, **{name: v if name != "ecc" else dict(pair).get("inner", 0)}) == want, (pair, name)
    # the back-off and the tap window (include/ofdm_hip.h): 3 cp_len / 4 = 12 at n_fft = 64
    for mode in (dict(chest_mode=cc.WLS), dict(cfo_mode=cc.CFO_WIDE)):
        assert [_create(lib, sync_backoff=b, **mode) for b in (0, 11, 12, 16)] == [want, want, -1, -1], mode
    assert _create(lib, sync_backoff=16, chest_mode=cc.WLS, sync_mode=cc.REFERENCE) == want
    assert _create(lib, sync_backoff=16) == want
    for k in cc.cases():
        assert _create(lib, k) == want, k.id


# ---------------------------------------------------------------------------------------------------------- 3. transmit
def test_mode_encode_has_the_length_of_the_mode():
    assert len(chain_refs.ALL_MODES) == 30
    rng = np.random.default_rng(3)
    for ecc in chain_refs.ALL_MODES:
        for p in (0, 1, 100, 300):
            pay = bytes(rng.integers(0, 256, p, dtype=np.uint8))
            assert len(rr.mode_encode(ecc, pay)) == chain_refs.mode_coded_len(ecc, p), (ecc, p)
    # every ecc of the table is one of the library's modes
    assert {k.ecc for k in cc.cases()} <= set(chain_refs.ALL_MODES)


# ---------------------------------------------------------------------------------------------------------- 4. the link
def test_every_row_has_a_seed_whose_captures_lock(orc):
    """cover_cases.seed_of: the first of the row's eight seeds for which the reference front end reports status 0 for all three frames
    and a frame start within [true delay - backoff - 2, true delay]"""
    none = []
    for k in cc.cases():
        seed = cc.seed_of(orc, k.index)
        print(f"row {k.index:2d} {k.id}: seed {seed}" + (f" (try {seed - k.first_seed + 1})" if seed is not None else ""))
        if seed is None:
            none.append(k.id)
    assert not none, none


def test_four_preamble_copies_leave_a_short_window_a_plateau(orc):
    """The finding behind cover_cases.Case.blanked_copies, on the first row with sync_window_reps = 1 that searches every lag: sent as
    the transmitter builds them, the frames of none of its eight seeds lock, and the timing is late by up to two periods -- the metric
    of a window of one period is 1 all along the two further copies.  Sent with the last two copies blanked, they lock."""
    k = next(k for k in cc.cases() if k.sync_mode == cc.SC and k.reps == 1 and k.n_lags == 0)
    assert k.blanked_copies() == 2
    main = int(np.argmax(np.abs(orc.channel_taps())))
    late = []
    for seed in range(k.first_seed, k.first_seed + cc.SEEDS_PER_ROW):
        ln = cc.link(orc, k.index, seed)
        whole = np.stack([cc.channel(orc, ln.tx[f], k.snr_db, np.random.default_rng(seed), int(ln.delay[f]), float(ln.f_delta[f]), ln.rx.shape[1])
                          for f in range(cc.FRAMES)])
        fe = rr.front_end(orc, whole, k, ln.D)
        late.append(max(f.offset - (int(ln.delay[i]) + main) for i, f in enumerate(fe)))
    print(f"{k.id}: frame start behind the true one, worst frame per seed: {late}; S = {k.S}")
    assert all(0 < v <= 2 * k.S for v in late)
    assert cc.seed_of(orc, k.index) is not None
