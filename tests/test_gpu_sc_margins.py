"""Every Schmidl-Cox detector family on razor-thin decisions (tests/sc_margin_cases.py): the threshold sits within 1e-6, 1e-9 and
eps_min = 1e-12 of a lag's own metric, below and above it, on an ordinary capture and behind bursts that leave the windows 2^-9,
2^-15 and 2^-17 of the capture's energy.  One Context per threshold, one sc_correlate call over the batch of a size's four captures per
search form; every row the CPU module has shown unambiguous is compared with orc.sc_sync at that threshold: d_hat equal, CFO to 1e-9,
metric to 1e-6 max(1, metric).  last_dispatch() must name the family under test.

Search forms.  `wide`: n_lags = d_k + W + 64, the bounded search of the case.  `all`: every lag of the capture, where a family is only
reached by a long search (the oracle's verdict is the same: a row is used when its window was not clipped by the bounded search).
`razor`: n_lags = d_k + 1 -- the razor lag is the last one searched, so the decision there IS the answer (d_k or -1); over more lags a
crossing found one lag late returns the same peak, and no detector error could show.  `tight`: the wide search on captures cut right
behind the last sample it reads."""
import functools

import numpy as np
import pytest

import sc_margin_cases as smc
from util import sc80_corner_captures, wide

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api(ofdm):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ofdm_amd import api as _api

    return _api


def host(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def all_lags_verdicts(orc, n, late=False):
    """{(threshold index, row): orc.sc_sync over every lag} for the rows whose bounded verdict it confirms"""
    sz = smc.build(orc, n, late)
    out = {}
    for ti, t in enumerate(sz.thresholds):
        for ci, bounded in enumerate(t.rows):
            if bounded is not None:
                want = orc.sc_sync(wide(sz.caps[ci]), sz.S, 3, 0, t.thr)
                if want[0] == bounded[0]:
                    out[ti, ci] = want
    assert len(out) >= 0.9 * sum(r is not None for t in sz.thresholds for r in t.rows)
    return out


def run_family(api, orc, n, tuning, forms, late=False, seen=None):
    """forms: {form: predicate on last_dispatch()} -> {(form, eps, capture): [rows compared, wrong ones]} after printing every wrong
    row; seen (a set): collects the dispatch strings"""
    sz = smc.build(orc, n, late)
    xd = None
    tally = {(form, eps, ci): [0, 0] for form in forms for eps in smc.EPS_FIXED + (sz.eps_min,) for ci in range(len(smc.CAPTURES))}
    bad = []
    for ti, t in enumerate(sz.thresholds):
        ctx = api.Context(n_fft=n, modulation=api.QAM16, guard_bands=True, sync_threshold=t.thr, tuning=tuning)
        xd = ctx.to_device(sz.caps) if xd is None else xd
        for form, names_family in forms.items():
            if form == "wide":
                got, want = ctx.sc_correlate(xd, n_lags=t.n_lags), dict(enumerate(t.rows))
            elif form == "razor":
                got, want = ctx.sc_correlate(xd, n_lags=t.d + 1), dict(enumerate(t.razor))
            elif form == "tight":
                flen = (t.n_lags + sz.W + sz.S) // 2 * 2
                got, want = ctx.sc_correlate(xd, frame_len=flen, n_lags=t.n_lags), dict(enumerate(t.rows))
            else:
                got = ctx.sc_correlate(xd)
                want = {ci: all_lags_verdicts(orc, n, late).get((ti, ci)) for ci in range(len(smc.CAPTURES))}
            disp = ctx.last_dispatch()
            assert names_family(disp), (n, tuning, form, disp)
            if seen is not None:
                seen.add(disp)
            d_hat, f_delta, metric = (host(v) for v in got)
            for ci, w in want.items():
                if w is None:
                    continue
                wd, _, wm, wfd = w
                good = d_hat[ci] == wd and (wd < 0 or (abs(f_delta[ci] - wfd) <= 1e-9 and abs(metric[ci] - wm) <= 1e-6 * max(1.0, wm)))
                tally[form, t.eps, ci][0] += 1
                tally[form, t.eps, ci][1] += not good
                if not good:
                    bad.append((form, smc.CAPTURES[ci], t.d, t.eps, t.sign, int(d_hat[ci]), wd))
    for b in bad:
        print("wrong:", n, tuning, *b)
    for form in forms:
        print(f"N = {n}{' late' if late else ''} {tuning} {form}: wrong / compared rows per eps and capture {smc.CAPTURES}: "
              + ", ".join(f"eps {eps:.0e}: {['%d/%d' % (tally[form, eps, ci][1], tally[form, eps, ci][0]) for ci in range(len(smc.CAPTURES))]}"
                          for eps in smc.EPS_FIXED + (sz.eps_min,)))
    return tally


def assert_exact(tally, but=()):
    """every row of every (form, eps, capture) is the oracle's, except the triples in `but` (stated where they are excused)"""
    assert all(compared > 0 for compared, _ in tally.values()), tally
    wrong = {key: w for key, (_, w) in tally.items() if w and key not in but}
    assert not wrong, wrong


starts = lambda *prefixes: (lambda disp: disp.startswith(prefixes))
equals = lambda name: (lambda disp: disp == name)


@pytest.mark.parametrize("tuning", [{}, {"grid_cap": 2}, {"sc80_depth": 1}], ids=["default", "grid_cap2", "depth1"])
def test_sc80(api, orc, tuning):
    """k_sc80 (f64 prefix differences): a decision inside the prefixes' error bound goes to the slow list, so every case is the oracle's"""
    forms = {"wide": starts("k_sc80"), "razor": starts("k_sc80")}
    if not tuning:
        forms["tight"] = starts("k_sc80")
    assert_exact(run_family(api, orc, 64, tuning, forms))


def test_sc80_keeps_ordinary_frames_off_the_slow_list(api, orc):
    ordinary, _ = sc80_corner_captures(orc)
    for thr in (0.5, 0.37, 0.81):
        ctx = api.Context(modulation=api.QAM64, guard_bands=True, sync_threshold=thr)
        d_hat = host(ctx.sc_correlate(ctx.to_device(np.stack(ordinary)))[0])
        assert ctx.last_dispatch().startswith("k_sc80") and ctx.get_tuning("stat_sc_slow_frames") == 0, thr
        assert [int(d) for d in d_hat] == [orc.sc_sync(wide(c), 80, 3, 0, thr)[0] for c in ordinary]


def test_threshold_keeps_its_double(api):
    """ofdm_params.sync_threshold is a float; a threshold a float cannot hold reaches the searches as the double it is (laboratory key
    sync_threshold_bits), one a float holds stays in the params alone, and nothing outside (0, 1] is taken"""
    bits = lambda v: int(np.float64(v).view(np.int64))
    assert api.Context(sync_threshold=0.5).get_tuning("sync_threshold_bits") == 0
    ctx = api.Context(sync_threshold=0.37)
    assert ctx.get_tuning("sync_threshold_bits") == bits(0.37) != bits(np.float32(0.37))
    for bad in (1.5, -0.25, float("nan"), float("inf")):
        with pytest.raises(api.OfdmError):
            ctx.set_tuning("sync_threshold_bits", bits(bad))
    assert ctx.get_tuning("sync_threshold_bits") == bits(0.37)
    ctx.set_tuning("sync_threshold_bits", 0)
    assert ctx.get_tuning("sync_threshold_bits") == 0


def test_sc_cf_one_launch(api, orc):
    """k_sc_cf<256> over every lag (f32 filter, exact f64 decisions where it fires) and k_sc_cf<128>, which bounded searches take"""
    assert_exact(run_family(api, orc, 64, {"no_sc80": 1, "sc_first_lags": 0},
                            {"all": starts("k_sc_cf<256>+"), "wide": starts("k_sc_cf<128>+"), "razor": starts("k_sc_cf<128>+")}))


def test_sc_cf_two_launches(api, orc):
    assert_exact(run_family(api, orc, 64, {"no_sc80": 1}, {"all": starts("k_sc_cf<128,first>+k_sc_cf<256,list>")}))


def test_sc_cf_256_at_the_razor_lag(api, orc):
    """The late set: record lags beyond the 960 lags of a 128-chunk tile, so the search that ends at the razor lag -- the one form in
    which a wrong decision there shows -- is served by k_sc_cf<256> in one launch, and in two launches with sc_first_lags = 400"""
    seen = set()
    assert_exact(run_family(api, orc, 64, {"no_sc80": 1, "sc_first_lags": 0},
                            {"razor": starts("k_sc_cf<256>+", "k_sc_cf<128>+"), "wide": starts("k_sc_cf<256>+")}, late=True, seen=seen))
    assert "k_sc_cf<256>+k_sc_tile<list>" in seen, seen
    seen = set()   # (the first record lag lies just inside 960: its razor search is k_sc_cf<128>'s)
    assert_exact(run_family(api, orc, 64, {"no_sc80": 1, "sc_first_lags": 400},
                            {"razor": starts("k_sc_cf<128,first>+k_sc_cf<256,list>", "k_sc_cf<128>+")}, late=True, seen=seen))
    assert any(d.startswith("k_sc_cf<128,first>+k_sc_cf<256,list>") for d in seen), seen
    assert_exact(run_family(api, orc, 64, {}, {"razor": starts("k_sc80"), "wide": starts("k_sc80")}, late=True))


@pytest.mark.parametrize("n", [256, 1024, 2048])
def test_sc_stream(api, orc, n):
    """k_sc_stream, the default from N = 128 on (N = 2048: the long-period default).  Its sums at every 10th lag are f64 prefix
    differences, slid lag by lag from there, and its decisions carry no error bound yet: exact at 1e-6 and 1e-9 on every capture and at
    eps_min = 1e-12 while the windows hold 2^-9 of the capture's energy or more; behind the 2^-15 and 2^-17 bursts a decision within
    1e-12 of the threshold may differ from the oracle's and is not asserted (measured on an MI355X at each of N = 256, 1024, 2048: 2 of
    8 rows wrong behind the 2^-15 burst and 2 of 8 behind the 2^-17 burst, all in searches that end at the razor lag; docs/NOTES.md)."""
    eps_min = smc.build(orc, n).eps_min
    assert_exact(run_family(api, orc, n, {}, {"wide": starts("k_sc_stream"), "razor": starts("k_sc_stream")}),
                 but={("razor", eps_min, 2), ("razor", eps_min, 3)})


@pytest.mark.parametrize("big_tiles", [0, 1])
@pytest.mark.parametrize("n", [256, 1024])
def test_scb_chunks_and_fine(api, orc, n, big_tiles):
    """k_scb_chunks + k_scb_fine take searches over more than one k_sc_tile tile: every lag at N = 256, the bounded search at N = 1024"""
    name = f"k_scb_chunks<contig>+k_scb_fine<{10 if big_tiles else 5}>"
    assert_exact(run_family(api, orc, n, {"no_sc_stream": 1, "scb_big_tiles": big_tiles}, {"all" if n == 256 else "wide": equals(name)}))


def test_scb_chunks_and_fine_at_the_razor_lag(api, orc):
    """At N = 2048 the window of even the shortest search is more than k_sc_tile holds in 64 KiB of LDS, so the search that ends at the
    razor lag goes through k_scb_chunks + k_scb_fine too: the one form in which a wrong decision there shows.  k_scb_fine takes its
    boundary sums as f64 prefix differences of chunk totals and slides from there, without an error bound: exact at 1e-6 and 1e-9 on
    every capture and at eps_min = 1e-12 down to windows of 2^-15 of the capture's energy; behind the 2^-17 burst a decision within
    1e-12 of the threshold may differ and is not asserted (measured on an MI355X: 2 of 4 such rows; docs/NOTES.md)."""
    is_scb = lambda disp: disp.startswith("k_scb_chunks") and "+k_scb_fine<5>" in disp
    eps_min = smc.build(orc, 2048).eps_min
    assert_exact(run_family(api, orc, 2048, {"no_sc_stream": 1}, {"razor": is_scb, "wide": is_scb}), but={("razor", eps_min, 3)})


def test_sc_tile(api, orc):
    """k_sc_tile, direct f64 sums: the multi-tile form over the bounded search, one tile when the search ends at the razor lag"""
    assert_exact(run_family(api, orc, 1024, {"no_sc_stream": 1, "no_sc_big": 1},
                            {"wide": equals("k_sc_tile<cross>+k_sc_tile<peak>"), "razor": equals("k_sc_tile")}))
