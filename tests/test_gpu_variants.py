"""Every kernel variant that only a batch shape or a laboratory key of ofdm_set_tuning selects (ofdm_amd/csrc/ofdm_hip_tuning.h), each
run through the Python face, named by last_dispatch() -- no case can pass on the default kernel by accident --, compared with the
f64 oracle (or zlib) at the project's tolerances, and, where the variant is by construction the default's arithmetic, required to
equal the default's output bit for bit.  Tolerances: bytes, lags, statuses exact; CFO 1e-9; metric 1e-6 max(1, metric); complex samples
TOL norm-relative.  tests/test_variants_cpu.py keeps the list of keys and dispatch names complete."""
import functools

import numpy as np
import pytest

from util import (SC80_SEARCHES, assert_bytes_match, decision_margin, fc32, long_period_captures, loud_payload, make_symbols_np, rel_err,
                  sc80_corner_captures, through_channel, wide)

pytestmark = pytest.mark.gpu
TOL = 1e-5  # north_star tolerance for complex samples


@pytest.fixture(scope="module")
def api(ofdm):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ofdm_amd import api as _api

    return _api


def host(t):
    return t.cpu().numpy()


def same_bits(a, b):
    """two tuples of device tensors, equal bit for bit"""
    return all(np.array_equal(host(x).view(np.uint8), host(y).view(np.uint8)) for x, y in zip(a, b))


def assert_sc_is_the_oracle(got, want, what):
    """got: (d_hat, f_delta, metric) on the host; want: [orc.sc_sync(...)] per frame"""
    d_hat, f_delta, metric = got
    for f, (wd, _, wm, wfd) in enumerate(want):
        assert d_hat[f] == wd, (what, f, int(d_hat[f]), wd)
        if wd >= 0:
            assert abs(f_delta[f] - wfd) <= 1e-9 and abs(metric[f] - wm) <= 1e-6 * max(1.0, wm), (what, f)


# ------------------------------------------------------------------ 1. k_demod64: store bursts of 16 / 8 / 4 / 1 groups, store variants
@functools.lru_cache(maxsize=None)
def demod_pool(orc, nsym):
    """nsym N = 64, 64-QAM, guard-band symbols at 34 dB and the oracle's bytes and soft points.  No decision of the oracle lies near a
    boundary (asserted), so the kernels must give its bytes exactly: no excused decision."""
    rng = np.random.default_rng(6400 if nsym == 1152 else 6410)
    x, data = make_symbols_np(orc, rng, nsym, 64, True, 6, snr_db=34.0)
    want, wsoft = orc.rx_demod(wide(x), 64, True, 6, want_soft=True)
    assert want == data
    assert decision_margin(wsoft, 6).min() >= 1e-4
    return x, want, np.asarray(wsoft)


def demod64(api, orc, nsym_pool, frames, syms, tuning, want_kernel, rows_of=None, first_symbol=0):
    """frames x syms symbols of the pool through rx_demod (no soft output: k_demod64) under `tuning`; rows_of: symbols per input row when
    only syms of them, from first_symbol on, are demodulated -> the output tensor, after the dispatch and oracle checks"""
    x, want, wsoft = demod_pool(orc, nsym_pool)
    rows_of = rows_of or syms
    ctx = api.Context(n_fft=64, modulation=api.QAM64, guard_bands=True, tuning=tuning)
    xd = ctx.to_device(x[: frames * rows_of * 80]).reshape(frames, rows_of * 80)
    out = ctx.rx_demod(xd, syms_per_frame=syms, first_symbol=first_symbol)
    assert ctx.last_dispatch() == want_kernel, (ctx.last_dispatch(), want_kernel, frames, syms, tuning)
    assert out.is_contiguous() and out.data_ptr() % 128 == 0
    bps = ctx.bytes_per_symbol
    wsel = np.frombuffer(want, np.uint8)[: frames * rows_of * bps].reshape(frames, rows_of * bps)[:, first_symbol * bps:(first_symbol + syms) * bps]
    ssel = wsoft[: frames * rows_of * 48].reshape(frames, rows_of, 48)[:, first_symbol:first_symbol + syms].reshape(-1)
    excused = assert_bytes_match(bytes(host(out).ravel()), bytes(wsel.ravel()), ssel, 6, what=f"{want_kernel} {frames}x{syms} {tuning}")
    assert excused == 0
    return out


@pytest.mark.parametrize("frames,syms,grid_cap,want_kernel", [
    (4, 8, 0, "k_demod64<burst4>"),       # 4 groups: one burst, three idle wavefronts
    (4, 24, 0, "k_demod64<burst4>"),      # 12 groups, 3 a frame: bursts straddle frames
    (44, 24, 1, "k_demod64<burst4>"),     # 132 = 4 x 33 groups on one workgroup: 9 steps per wavefront, ragged last step
    (8, 24, 0, "k_demod64<burst8>"),      # 24 groups: a burst spans 2 2/3 frames
    (40, 24, 1, "k_demod64<burst8>"),     # 120 = 8 x 15 groups on one workgroup: 4 steps, ragged last
    (5, 16, 0, "k_demod64"),              # 10 groups: no multiple of 4, BURST = 1 of the same instantiation, wide stores
])
def test_demod64_burst_is_chosen_by_the_batch_shape(api, orc, frames, syms, grid_cap, want_kernel):
    """launch_demod64 (kernels_n64.hip) picks k_demod64<6,true,false,BURST> from the group count alone: 16 | groups -> 16, 8 | groups ->
    8, 4 | groups -> 4, else 1.  The burst loop has arithmetic of its own (one 64-bit division per burst, the frame / group wrap
    inside a burst, image offsets b * REGION_DW * 4, one store of BURST * REGION_DW dwords): every burst size against the oracle's
    bytes, exactly, with no key set and the output as torch allocates it."""
    demod64(api, orc, 1152, frames, syms, {"grid_cap": grid_cap}, want_kernel)


def test_demod64_burst_with_a_row_stride_larger_than_the_frame(api, orc):
    """symbols 8..15 of 12 rows of 24: 12 groups, one a frame, the input row stride three times the frame, the output contiguous -> burst4"""
    demod64(api, orc, 1152, 12, 8, {}, "k_demod64<burst4>", rows_of=24, first_symbol=8)


@pytest.mark.parametrize("tuning,want_kernel", [
    ({"demod64_burst": 8}, "k_demod64<burst8>"),
    ({"demod64_burst": 4}, "k_demod64<burst4>"),
    ({"demod64_burst": 1}, "k_demod64"),
    ({"demod64_narrow_stores": 1}, "k_demod64"),          # dword stores: no bursts either
    ({"demod64_store_policy": 1}, "k_demod64<burst16>"),  # nt
    ({"demod64_store_policy": 2}, "k_demod64<burst16>"),  # sc1
    ({"demod64_store_policy": 3}, "k_demod64<burst16>"),  # sc0 sc1
], ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_demod64_store_variants_by_key(api, orc, tuning, want_kernel):
    """48 x 24 symbols = 144 = 16 x 9 groups (burst16 by default) under every key that changes how k_demod64 stores its images.  The
    keys change which groups a wavefront takes and how the finished LDS image leaves (burst length, 4- or 16-byte stores, cache-policy
    bits), never a group's arithmetic: bit-identical to the default by construction, and equal to the oracle."""
    base = demod64(api, orc, 1152, 48, 24, {}, "k_demod64<burst16>")
    out = demod64(api, orc, 1152, 48, 24, tuning, want_kernel)
    assert same_bits((out,), (base,))


def test_demod64_one_workgroup_per_cu_wraps_the_grid(api, orc):
    """demod64_wg_per_cu = 1 with demod64_burst = 1: one workgroup (four groups a step) per CU and more than 8 groups per CU, so the
    persistent grid walks two whole steps and a ragged third (the host-supplied step_df / step_dk increments).  Sized from the device's
    CU count (688 x 24 on 256 CUs).  Only the grid differs from the default: bit-identical to it."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    frames = (8 * cus + 16 + 2) // 3                    # x 3 groups: two steps of 4 cus groups and a few more
    assert frames * 3 > 8 * cus and (frames * 3) % (4 * cus) != 0
    groups = frames * 3
    by_shape = "k_demod64<burst16>" if groups % 16 == 0 else "k_demod64<burst8>" if groups % 8 == 0 else "k_demod64<burst4>" if groups % 4 == 0 else "k_demod64"
    base = demod64(api, orc, frames * 24, frames, 24, {}, by_shape)
    out = demod64(api, orc, frames * 24, frames, 24, {"demod64_burst": 1, "demod64_wg_per_cu": 1}, "k_demod64")
    assert same_bits((out,), (base,))


# ------------------------------------------------------------------ 2. k_sc80<1>: sc80_depth = 1
@functools.lru_cache(maxsize=None)
def sc80_cases(orc):
    """the corner-case captures of k_sc80 (tests/util.py) and the oracle's verdict on every (capture, search) pair, computed once"""
    ordinary, dynamic = sc80_corner_captures(orc)
    want = {(f, s): orc.sc_sync(wide(ordinary[f][:flen]), 80, 3, n_lags, thr) for f in range(len(ordinary))
            for s, (thr, n_lags, flen) in enumerate(SC80_SEARCHES)}
    want_dyn = [orc.sc_sync(wide(c), 80, 3, 0, 0.5) for c in dynamic]
    return ordinary, dynamic, want, want_dyn


def sc80_pair(api, threshold=0.5, **tuning):
    """contexts with k_sc80<1> (sc80_depth = 1) and the default k_sc80<2>"""
    mk = lambda depth: api.Context(modulation=api.QAM64, guard_bands=True, sync_threshold=threshold, tuning={**tuning, "sc80_depth": depth})
    return mk(1), mk(2)


def test_sc80_depth_one_on_the_corner_cases(api, orc):
    """k_sc80<1> keeps 9 - 10 ring pieces in flight instead of 7: another hand-counted s_waitcnt vmcnt schedule and another refill
    order, over the same ring and the same arithmetic.  If the schedule is right every step reads the same samples, so the depth only
    changes WHEN loads are issued: bit-identical to sc80_depth = 2 by construction, on top of the oracle's lag, CFO and metric.
    Ragged batches on a capped grid, other thresholds, bounded and short searches; the dynamic-range captures (slow list)."""
    ordinary, dynamic, want, want_dyn = sc80_cases(orc)
    for nfr in (1, 3, 13):
        caps = np.stack(ordinary[:nfr])
        for s, (thr, n_lags, flen) in enumerate(SC80_SEARCHES):
            one, two = sc80_pair(api, thr, grid_cap=2)
            got = one.sc_correlate(one.to_device(caps), frame_len=flen, n_lags=n_lags)
            assert one.last_dispatch().startswith("k_sc80") and one.last_dispatch() == "k_sc80+k_sc_tile<list>", one.last_dispatch()
            assert_sc_is_the_oracle([host(t) for t in got], [want[f, s] for f in range(nfr)], (nfr, thr, n_lags, flen))
            ref = two.sc_correlate(two.to_device(caps), frame_len=flen, n_lags=n_lags)
            assert two.last_dispatch() == "k_sc80+k_sc_tile<list>"
            assert same_bits(got, ref), (nfr, thr, n_lags, flen)
    one, two = sc80_pair(api)
    got = one.sc_correlate(one.to_device(dynamic))
    assert one.last_dispatch().startswith("k_sc80"), one.last_dispatch()
    slow = one.get_tuning("stat_sc_slow_frames")
    assert 2 <= slow <= 3, slow                          # the gap and the quiet packet (the hot one may or may not be trusted)
    assert_sc_is_the_oracle([host(t) for t in got], want_dyn, "dynamic range")
    ref = two.sc_correlate(two.to_device(dynamic))
    assert two.get_tuning("stat_sc_slow_frames") == slow and same_bits(got, ref)


def test_sc80_depth_one_restarts_its_ring_on_long_slots(api, orc):
    """514 slots of 6 000 samples (more than a dozen laps of the 480-sample ring; long slots take k_sc80 from 512 rows on) on ONE wavefront:
    129 groups, the ring restarted for each, the last group half empty.  A packet near sample 3 000, a noise-only slot (streamed to its
    end) and an early packet (the stream stops after a lap or two) side by side in every group."""
    rng = np.random.default_rng(8081)
    span, nfr = 6000, 514
    tx = orc.encode(bytes(rng.integers(0, 256, 560, dtype=np.uint8)), True, orc.QAM64)
    kinds = np.stack([through_channel(orc, rng, tx, span, 3011, 0.021, 30.0),
                      fc32(0.004 * (rng.standard_normal(span) + 1j * rng.standard_normal(span))),
                      through_channel(orc, rng, tx, span, 37, -0.013, 30.0)])
    want3 = [orc.sc_sync(wide(c), 80, 3, 0, 0.5) for c in kinds]
    assert want3[0][0] == 3011 + 89 and want3[1][0] == -1 and want3[2][0] == 37 + 89
    caps = kinds[np.arange(nfr) % 3]
    one, two = sc80_pair(api, grid_cap=1)
    got = one.sc_correlate(one.to_device(caps))
    assert one.last_dispatch().startswith("k_sc80"), one.last_dispatch()
    assert one.last_dispatch() == "k_sc80+k_sc_tile<list,cross>+k_sc_tile<list,peak>"
    assert one.get_tuning("stat_sc_slow_frames") == 0
    assert_sc_is_the_oracle([host(t) for t in got], [want3[f % 3] for f in range(nfr)], "long slots")
    assert same_bits(got, two.sc_correlate(two.to_device(caps)))


# ------------------------------------------------------------------ 3. k_sc_cf<128,1,5> (sc128_one_wave = 0) and the filter pair's grid (sc_wg_per_cu)
@functools.lru_cache(maxsize=None)
def sc128_cases(orc):
    """13 N = 64 captures of 2 176 samples: packets at delays 1 .. 79, at 300 and 420 (their peak windows reach beyond the first 576
    lags), one noise-only; the oracle over every lag, and bounded to 300 and to 45 lags of the first 2 000 samples"""
    rng = np.random.default_rng(128)
    span = 2176
    tx = orc.encode(bytes(rng.integers(0, 256, 560, dtype=np.uint8)), True, orc.QAM64)
    delays = [1, 2, 9, 17, 26, 35, 44, 53, 66, 79, 300, 420]
    caps = [through_channel(orc, rng, tx, span, d, float((rng.random() * 1.9 - 0.95) * np.pi / 80), 30.0) for d in delays]
    caps.append(fc32(0.05 * (rng.standard_normal(span) + 1j * rng.standard_normal(span))))
    caps = np.stack(caps)
    want = {(n_lags, flen): [orc.sc_sync(wide(c[:flen]), 80, 3, n_lags, 0.5) for c in caps] for n_lags, flen in ((0, span), (300, 2000), (45, 2000))}
    assert [w[0] for w in want[0, span][:12]] == [d + 89 for d in delays] and want[0, span][12][0] == -1
    return caps, want


def sc128_run(api, caps, want, tuning):
    """the whole search (two launches) and the two bounded searches under `tuning` + no_sc80 -> their results, after the dispatch and
    oracle checks"""
    ctx = api.Context(modulation=api.QAM64, guard_bands=True, tuning={"no_sc80": 1, **tuning})
    xd = ctx.to_device(caps)
    out = []
    for (n_lags, flen), w in want.items():
        got = ctx.sc_correlate(xd, frame_len=flen, n_lags=n_lags)
        disp = ctx.last_dispatch()
        if n_lags == 0:
            assert "k_sc_cf<128,first>" in disp and "k_sc_cf<256,list>" in disp, disp
            assert ctx.get_tuning("stat_sc_redo_frames") >= 3            # the two late packets and the noise-only slot
        else:
            assert "k_sc_cf<128>" in disp and disp == "k_sc_cf<128>+k_sc_tile<list>", disp
        assert_sc_is_the_oracle([host(t) for t in got], w, (tuning, n_lags, flen))
        out.append(got)
    return out


def test_sc128_two_waves_per_frame_and_grid_sizing(api, orc):
    """sc128_one_wave = 0 runs the 128-chunk filter as k_sc_cf<128,1,5>: 128 threads with a chunk each instead of 64 with two, in the
    first launch of the two-launch search and in bounded searches.  A thread's chunks are laid out so that every (wavefront, u) pair is
    the same run of 64 consecutive chunks in both instantiations -- the f32 scans add in the same order -- and decisions are exact f64
    either way: bit-identical to sc128_one_wave = 1 by construction.  sc_wg_per_cu (1, 16) only sizes the persistent grid of
    k_sc_cf<256,list>: identical results."""
    caps, want = sc128_cases(orc)
    base = sc128_run(api, caps, want, {"sc128_one_wave": 1})
    two = sc128_run(api, caps, want, {"sc128_one_wave": 0})
    for a, b in zip(two, base):
        assert same_bits(a, b)
    for per_cu in (1, 16):
        for a, b in zip(sc128_run(api, caps, want, {"sc_wg_per_cu": per_cu}), base):
            assert same_bits(a, b), per_cu


# ------------------------------------------------------------------ 4. long periods through the two-pass kernels' other forms
@pytest.mark.parametrize("n,mod,nbytes", [(128, 4, 300), (1024, 6, 1304)])
def test_long_period_two_segment_staging_and_tile_search(api, orc, n, mod, nbytes):
    """no_sc_stream = 1 with scb_two_segments = 1: k_scb_chunks<false> (the tile and its partner tile L samples later as two LDS
    segments) at L = 160 and at L = 1 280, the edge of the contiguous form's range, where only longer periods take it by default; with
    no_sc_big = 1: the k_sc_tile family (one tile, or first crossing per tile + peak).  Five frames, noise only, a capture cut inside
    the preamble; every lag, a search bounded to 2 S lags (one k_sc_tile tile with the window in LDS: the launcher sends that to
    k_sc_tile whatever the keys say) and one bounded to 2 560 + S lags (more than a tile: the chunk kernels again).  Against the oracle;
    d_hat equal to the default streaming detector's.  The two stagings sum the same micro-chunks in the same order, so the
    two-segment form is also bit-identical to the contiguous one.

    (The cut capture at N = 128 over every lag is what k_scb_fine once got wrong, in both stagings: behind the capture's end a window of
    zeros slid along a tile came out as rounding residue, residue / residue = 0.643 at lag 570 beat the true peak 0.577 at lag 180.)"""
    rng = np.random.default_rng(7100 + n)
    S = n + n // 4
    mk = lambda tuning: api.Context(n_fft=n, modulation=mod, guard_bands=True, tuning=tuning)
    stream, contig = mk({}), mk({"no_sc_stream": 1})
    seg, tile = mk({"no_sc_stream": 1, "scb_two_segments": 1}), mk({"no_sc_stream": 1, "no_sc_big": 1})
    span = max(stream.frame_samples(nbytes) + 3 * S // 2, 2560 + 5 * S + 2) // 2 * 2
    caps = long_period_captures(orc, rng, n, mod, nbytes, 5, span)
    for lags in (0, 2 * S, 2560 + S):
        want = [orc.sc_sync(wide(c), L=S, window_reps=3, n_lags=lags, threshold=0.5) for c in caps]
        one_tile = 0 < lags <= 2560
        d0 = host(stream.sc_correlate(stream.to_device(caps), n_lags=lags)[0])
        assert stream.last_dispatch() == ("k_sc_stream<regs>" if n == 1024 else "k_sc_stream")
        ref = contig.sc_correlate(contig.to_device(caps), n_lags=lags)
        assert contig.last_dispatch() == ("k_sc_tile" if one_tile else "k_scb_chunks<contig>+k_scb_fine<5>")
        assert_sc_is_the_oracle([host(t) for t in ref], want, ("no_sc_stream", n, lags))
        got = seg.sc_correlate(seg.to_device(caps), n_lags=lags)
        assert seg.last_dispatch() == ("k_sc_tile" if one_tile else "k_scb_chunks+k_scb_fine<5>"), (seg.last_dispatch(), lags)
        assert_sc_is_the_oracle([host(t) for t in got], want, ("scb_two_segments", n, lags))
        assert np.array_equal(host(got[0]), d0) and same_bits(got, ref)
        got = tile.sc_correlate(tile.to_device(caps), n_lags=lags)
        assert tile.last_dispatch() == ("k_sc_tile" if one_tile else "k_sc_tile<cross>+k_sc_tile<peak>"), (tile.last_dispatch(), lags)
        assert "k_scb" not in tile.last_dispatch()
        assert_sc_is_the_oracle([host(t) for t in got], want, ("no_sc_big", n, lags))
        assert np.array_equal(host(got[0]), d0)
    assert sum(w[0] >= 0 for w in want) >= 5


# ------------------------------------------------------------------ 5. k_txframe_mid two-pass on one-step frames, k_txframe64 grid
@pytest.mark.parametrize("n,mod,D", [(512, 2, 3), (2048, 4, 1)])
def test_txframe_mid_builds_one_step_frames_twice(api, orc, n, mod, D):
    """txframe_keep_steps = 0 sends frames whose data symbols fit one workgroup step (N >= 512: built once, points kept in registers,
    by default) through the two-pass k_txframe_mid<R, GUARD, 0>: N = 512 with D = 3 (R = 8, four symbols a step: four frames share a
    round), N = 2048 with D = 1 (R = 32).  11 ragged payloads on two workgroups; at N = 512 two of them louder than their header, so a
    round shared by loud and ordinary frames is rebuilt (a one-symbol frame's only symbol starts with the length header: it cannot be
    made loud with util.loud_payload).  Both forms run the same symbol builder and scale by the same (1 / N) / max(header, frame)
    expression: bit-identical to the default by construction, with and without no_txframe_optimistic."""
    import torch
    rng = np.random.default_rng(5000 + n)
    nbytes = D * (n * mod // 8) - 16
    nfr = 11
    S = n + n // 4
    lens = rng.integers(0, nbytes + 1, nfr).astype(np.int32)
    lens[0], lens[-1] = nbytes, 0
    pay = rng.integers(0, 256, (nfr, nbytes), dtype=np.uint8)
    loud = (2, 5) if D > 1 else ()
    for i, f in enumerate(loud):
        pay[f], lens[f] = loud_payload(orc, n, mod, nbytes, 1 + i, seed=f), nbytes
    want = [orc.encode(bytes(pay[f, :lens[f]]), False, mod, n) for f in range(nfr)]
    assert sum(max(w[:10 * S].real.max(), w[:10 * S].imag.max()) < 0.5 for w in want) == len(loud)
    run = lambda tuning: api.Context(n_fft=n, modulation=mod, guard_bands=False, tuning={"grid_cap": 2, **tuning})
    base = run({})
    assert base.data_symbols(nbytes) == D
    fbase = base.encode_batch(base.to_device(pay), lens=torch.from_numpy(lens))
    assert base.last_dispatch() == "k_txframe_mid<once>"
    for tuning in ({"txframe_keep_steps": 0}, {"txframe_keep_steps": 0, "no_txframe_optimistic": 1}):
        ctx = run(tuning)
        frames = ctx.encode_batch(ctx.to_device(pay), lens=torch.from_numpy(lens))
        assert ctx.last_dispatch() == "k_txframe_mid", (ctx.last_dispatch(), tuning)
        assert same_bits((frames,), (fbase,)), tuning
        frames = host(frames)
        assert frames.shape == (nfr, (10 + D) * S)
        for f in range(nfr):
            assert rel_err(frames[f, :want[f].size], want[f]) <= TOL, (tuning, f, int(lens[f]))
            assert abs(max(frames[f].real.max(), frames[f].imag.max()) - 1.0) < 1e-6, (tuning, f)


@pytest.mark.parametrize("waves", [1, 32])
def test_txframe64_wavefronts_per_cu(api, orc, waves):
    """tx_waves only sizes k_txframe64's persistent grid (wavefronts per CU): 9 ragged N = 64 frames, bit-identical to the default's
    16 and equal to the oracle"""
    import torch
    rng = np.random.default_rng(64 + waves)
    nbytes, nfr = 560, 9
    lens = rng.integers(0, nbytes + 1, nfr).astype(np.int32)
    lens[0], lens[-1] = nbytes, 0
    pay = rng.integers(0, 256, (nfr, nbytes), dtype=np.uint8)
    base = api.Context(n_fft=64, modulation=api.QAM64, guard_bands=True)
    ctx = api.Context(n_fft=64, modulation=api.QAM64, guard_bands=True, tuning={"tx_waves": waves})
    fbase = base.encode_batch(base.to_device(pay), lens=torch.from_numpy(lens))
    frames = ctx.encode_batch(ctx.to_device(pay), lens=torch.from_numpy(lens))
    assert ctx.last_dispatch() == base.last_dispatch() == "k_txframe64"
    assert same_bits((frames,), (fbase,))
    frames = host(frames)
    for f in range(nfr):
        want = orc.encode(bytes(pay[f, :lens[f]]), True, api.QAM64)
        assert rel_err(frames[f, :want.size], want) <= TOL, f
