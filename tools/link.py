"""The one seeded link, the one speed capture and the bookkeeping that every mode's GPU tests (tests/test_gpu_*.py) and bench tool
(tools/bench_*.py) share.  A figure a test's comment quotes from a tool's record rests on both calling the functions here.

The order and the shapes of the generator's draws are part of the definition: every seed in the tests and in the committed records
(profiles/*_ber_and_speed.json) stands for one capture, and changing a draw changes them all.  ofdm_amd is imported inside the
functions, so collecting the tests on a machine without the library stays possible."""
import json
import math
import os

import numpy as np
import torch


# ---------------------------------------------------------------------------------------------------------- the seeded link
def data_snr(n, snr):
    # ofdm_channel_batch scales its noise by the whole frame's pseudo-variance, which the real-valued locking block dominates more the
    # larger N is (data samples ~ 1/sqrt(N)): the data symbols see ~10 log10(N / 64) dB less than the channel's snr_db
    return snr + 10.0 * np.log10(n / 64)


def generator(c, seed):
    g = torch.Generator(device=c.device)
    g.manual_seed(seed)
    return g


def seeded_channel(c, tx, snr, seed, g):
    """tx [n_frames, frame] through ofdm_channel_batch with one channel seed: per frame a delay of 1 .. 32 samples, then a CFO within
    +-1 / S rad/sample, drawn from g in that order; the capture is 160 samples longer than the frame"""
    n_frames = tx.shape[0]
    d = torch.randint(1, 33, (n_frames,), dtype=torch.int32, device=c.device, generator=g)
    fd = (torch.rand((n_frames,), dtype=torch.float64, device=c.device, generator=g) - 0.5) * (2.0 / c.S)
    return c.channel_batch(tx, snr_db=snr, seed=seed, delay=d, f_delta=fd, span=tx.shape[1] + 160)


def wide_channel(c, tx, snr, seed, g, span=8, m=None):
    """(rx, m, f_delta): seeded_channel for EXT-8, wide CFO acquisition -- per frame a delay of 1 .. 32 samples, then m uniform in
    [-span, span] (m given: that tensor, nothing drawn for it), then a fractional part within +-0.95 pi / S, drawn from g in that order;
    the channel turns by f_delta = the fractional part + 2 pi m / S, which no Schmidl-Cox phase alone can report for m != 0.  The capture
    is 160 samples longer than the frame.  seeded_channel's own draws are untouched."""
    n_frames = tx.shape[0]
    d = torch.randint(1, 33, (n_frames,), dtype=torch.int32, device=c.device, generator=g)
    if m is None:
        m = torch.randint(-span, span + 1, (n_frames,), dtype=torch.int32, device=c.device, generator=g)
    frac = (torch.rand((n_frames,), dtype=torch.float64, device=c.device, generator=g) * 1.9 - 0.95) * math.pi / c.S
    fd = frac + 2.0 * math.pi * m.to(torch.float64) / c.S
    return c.channel_batch(tx, snr_db=snr, seed=seed, delay=d, f_delta=fd, span=tx.shape[1] + 160), m, fd


def wide_link_on(c, n_frames, payload, snr, seed, span=8, m=None):
    """(pay, rx, m, f_delta): link_on through wide_channel"""
    g = generator(c, seed)
    pay = torch.randint(0, 256, (n_frames, max(payload, 1)), dtype=torch.uint8, device=c.device, generator=g)[:, :payload].contiguous()
    rx, m, fd = wide_channel(c, c.encode_batch(pay), snr, seed, g, span, m)
    return pay, rx, m, fd


def link_on(c, n_frames, payload, snr, seed):
    """(pay, rx): seeded payloads [n_frames, payload] encoded by context c and sent through seeded_channel; `seed` seeds both the
    generator and the channel.  The payloads are drawn max(payload, 1) wide, so a payload of 0 bytes draws what one of 1 byte does."""
    g = generator(c, seed)
    pay = torch.randint(0, 256, (n_frames, max(payload, 1)), dtype=torch.uint8, device=c.device, generator=g)[:, :payload].contiguous()
    return pay, seeded_channel(c, c.encode_batch(pay), snr, seed, g)


def link(ecc, n, mod, n_frames, payload, snr, seed, guard=True, **ctx_kw):
    """(context, pay, rx, data symbols of the frame): link_on over a new context (ctx_kw: chest_mode = ...)"""
    from ofdm_amd import api

    c = api.Context(n_fft=n, modulation=mod, guard_bands=guard, ecc=ecc, **ctx_kw)
    pay, rx = link_on(c, n_frames, payload, snr, seed)
    return c, pay, rx, c.data_symbols(payload)


def branch_link_on(c, n_frames, payload, snrs, seed):
    """(pay, rx [n_frames, R, span]): R = len(snrs) captures of every frame (EXT-7 soft combining) -- the payloads drawn as link_on draws
    them, ONE transmit frame each, then branch r through seeded_channel at snrs[r] with the channel seed `seed + r`, its delays and
    CFOs drawn from the generator branch after branch"""
    g = generator(c, seed)
    pay = torch.randint(0, 256, (n_frames, max(payload, 1)), dtype=torch.uint8, device=c.device, generator=g)[:, :payload].contiguous()
    tx = c.encode_batch(pay)
    return pay, torch.stack([seeded_channel(c, tx, snr, seed + r, g) for r, snr in enumerate(snrs)], dim=1).contiguous()


# ---------------------------------------------------------------------------------------------------------- what was delivered
def delivered(r, pay, want_len, exact=True):
    """(right, ok) masks over the frames of a decode_batch result: ok = status 0, right = ok with the length want_len (exact=False: at
    least want_len, for a mode that delivers its padding too) and the payload's bytes in front"""
    ok = r["status"] == 0
    length_ok = (r["len"] == want_len) if exact else (r["len"] >= want_len)
    return ok & length_ok & (r["bytes"][:, :pay.shape[1]] == pay).all(dim=1), ok


def bit_errors(diff):
    """set bits of a uint8 tensor (payload XOR delivered bytes)"""
    return int(sum(int(((diff >> b) & 1).sum()) for b in range(8)))


# ---------------------------------------------------------------------------------------------------------- speed
def capture(c, g, n_frames, pay, span, seed):
    """the 40 dB capture of the speed blocks, [n_frames, span]: chunks of 8192 frames, per chunk delays 1 .. 64 and a CFO within
    +-0.95 pi / S drawn from g, the channel seeded seed + the chunk's first frame"""
    x = torch.empty((n_frames, span), dtype=torch.complex64, device=c.device)
    chunk = 8192
    for lo in range(0, n_frames, chunk):
        hi = min(lo + chunk, n_frames)
        tx = c.encode_batch(pay[lo:hi].contiguous())
        d = torch.randint(1, 65, (hi - lo,), device=c.device, generator=g, dtype=torch.int32)
        fd = (torch.rand((hi - lo,), device=c.device, generator=g, dtype=torch.float64) * 1.9 - 0.95) * math.pi / c.S
        c.channel_batch(tx, snr_db=40.0, seed=seed + lo, delay=d, f_delta=fd, out=x[lo:hi])
        del tx
    torch.cuda.synchronize()
    return x


def alternated_ms(runs, reps):
    """runs: {name: (context, callable)}.  Every callable once as a warm-up (workspaces grown, code objects loaded), then `reps`
    rounds of all of them in turn, each between its context's timer_start / timer_stop_ms -> {name: [ms per round]}"""
    for _, f in runs.values():
        f()
    torch.cuda.synchronize()
    ms = {name: [] for name in runs}
    for _ in range(reps):
        for name, (c, f) in runs.items():
            c.timer_start(); f(); ms[name].append(c.timer_stop_ms())
    return ms


def median(v):
    return sorted(v)[len(v) // 2]


# ---------------------------------------------------------------------------------------------------------- the record
def save_record(rec, path):
    """rec to `path` (None: nowhere) through a .tmp file: a run that is cut short while it writes leaves the earlier file whole"""
    if path:
        with open(path + ".tmp", "w") as f:
            json.dump(rec, f, indent=1)
        os.replace(path + ".tmp", path)


def open_record(rec, path, keep_earlier=False):
    """(rec, save) for a tool that saves after every block, so that a run that is cut short keeps the blocks it has finished.
    keep_earlier: blocks of an earlier call's record at `path` stay unless this call measures them again."""
    if keep_earlier and path and os.path.exists(path):
        with open(path) as f:
            rec = {**json.load(f), **rec}
    return rec, lambda: save_record(rec, path)
