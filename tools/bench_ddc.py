#!/usr/bin/env python3
"""EXT-16 measurements: the digital down-converter (k_ddc) alone, one process on one MI355X -> profiles/ddc_speed.json.  No ratio is
fixed in advance: nobody had measured this kernel.

kernel   ofdm_ddc_push / _push_sc16 of 1 Mi, of 16 Mi and of 64 Mi input samples in ONE piece (max_chunk = the push), fc32 and sc16, D = 4 with
         T = 96 and D = 8 with T = 192 (the default design), next to
           - ofdm_hbm_read_probe (unit-stride 16-byte loads) over the bytes of the fc32 input, and
           - the time the FMA count alone would take: 2 T / D filter FMAs and 4 mixer FMAs (8 multiply-adds, half of them fused) an
             input sample, at `--f32-tflops` (default 78.6: 256 CUs x 4 SIMDs x 16 lanes x 2 flops x 2.4 GHz, plain v_fma_f32),
         the context's event timer, every way alternated in this one process, `--reps` passes each after a warm-up, medians with spread.
         The 16 Mi fc32 input (134 MB) fits the card's 256 MB memory-side cache and is read again on every pass: there the probe's figure
         is a CACHE bandwidth.  The 64 Mi input (537 MB) does not fit: that block is the one to hold against memory.
host     api.ddc_host over the same 16 Mi samples, D = 4: the "before", wall clock.  The host definition is one loop on one thread; the
         figure for `--host-threads` (16) threads runs it on that many equal slices at once (ctypes releases the interpreter lock) --
         a slice starts its own phase at 0, so this is a timing, not the stream's bits -- next to the one-thread figure.
stream   tools/bench_stream.py's two captures (`--samples` samples of tools/link.py's seeded link, 64-QAM with guard bands at 30 dB; N = 64
         and N = 1024), interpolated by 4 on the CPU (a Blackman-windowed sinc of 32 taps a phase) and shifted to f0 = 1 / 4, pushed
         through a stream with the converter in chunks of 16 Ki / 256 Ki / 4 Mi INPUT samples, alternated with the narrow-band capture
         through a plain stream in chunks of a quarter of that (bench_stream.py's own passes), wall clock around reset + every push +
         flush.  Asserted in the same run: the stream with the converter delivers the packets of ONE decode_all_host call on
         ddc_host(capture), every field bit for bit.
Whatever a call does not run stays "NOT YET MEASURED" in the record.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ofdm_amd import api  # noqa: E402
from tools.bench_scan import stat, wall_alternated  # noqa: E402
from tools.bench_stream import FIELDS, same_packets  # noqa: E402
from tools.link import alternated_ms, link, open_record  # noqa: E402

NOT_YET = "NOT YET MEASURED"
SHAPES = ((4, 96), (8, 192))
CHUNKS = (16384, 262144, 1 << 22)   # input samples
STREAM_D = 4
INTERP_TPP = 32


def kernel_block(n, reps, tflops):
    c = api.Context(n_fft=64, modulation=api.QAM64, guard_bands=True)
    g = torch.Generator(device="cpu").manual_seed(n % 1000)
    x = c.to_device((torch.randn(n, 2, generator=g) * 0.1).numpy().view(np.complex64).reshape(-1))
    q = c.to_device(torch.randint(-20000, 20000, (n, 2), generator=g, dtype=torch.int16).numpy())
    out = c.empty((n // 4 + 8,), torch.complex64)
    probe = x[: n // 80 * 80]
    rec = {"samples": n, "hbm_read_probe_bytes": 8 * (n // 80 * 80)}
    handles = {(D, T): c.ddc(D, api.ddc_inc_for(1.0 / D), api.ddc_design(D), max_chunk=n) for D, T in SHAPES}
    runs = {"hbm_read_probe": (c, lambda: c.hbm_read_probe(probe, 2))}

    def once(f, src, scale):
        def go():
            f.reset()
            f.push(src, scale=scale, out=out)
        return go

    for (D, T), f in handles.items():
        runs["fc32_D%d_T%d" % (D, T)] = (c, once(f, x, None))
        runs["sc16_D%d_T%d" % (D, T)] = (c, once(f, q, 1.0 / 32768))
    ms = alternated_ms(runs, reps)
    for k, v in ms.items():
        s = stat(v)
        if k == "hbm_read_probe":
            rec[k] = {**s, "bytes_moved": rec["hbm_read_probe_bytes"], "gb_per_s": round(rec["hbm_read_probe_bytes"] / s["ms_median"] / 1e6, 1)}
            continue
        D, T = (int(t[1:]) for t in k.split("_")[1:])
        fma = (2 * T // D + 4) * n                       # per input sample: T / D taps x 2 parts, 4 fused of the mixer's 8 products
        nbytes = (8 if k.startswith("fc32") else 4) * n + 8 * (n // D)
        rec[k] = {**s, "bytes_moved": nbytes, "gb_per_s": round(nbytes / s["ms_median"] / 1e6, 1), "gsamples_per_s": round(n / s["ms_median"] / 1e6, 2),
                  "fma_count": fma, "fma_alone_ms": round(2 * fma / (tflops * 1e12) * 1e3, 4),
                  "fma_tflops_reached": round(2 * fma / s["ms_median"] / 1e9, 2)}
    f = handles[SHAPES[0]]
    f.reset()
    f.push(x, out=out)
    assert c.last_dispatch() == "k_ddc<fc32>"
    for f in handles.values():
        f.close()
    return rec


def host_block(n, threads):
    from concurrent.futures import ThreadPoolExecutor

    rng = np.random.default_rng(1)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    h, inc = api.ddc_design(4), api.ddc_inc_for(0.25)
    api.ddc_host(x[: 1 << 16], 4, 5, h)
    t = time.perf_counter()
    api.ddc_host(x, 4, inc, h)
    one = time.perf_counter() - t
    step = n // threads
    with ThreadPoolExecutor(threads) as ex:
        t = time.perf_counter()
        list(ex.map(lambda i: api.ddc_host(x[i * step: (i + 1) * step], 4, inc, h), range(threads)))
        many = time.perf_counter() - t
    return {"samples": n, "decim": 4, "taps": 96,
            "one_thread": {"seconds": round(one, 3), "msamples_per_s": round(n / one / 1e6, 2)},
            "threads_%d" % threads: {"seconds": round(many, 3), "msamples_per_s": round(n / many / 1e6, 2),
                                     "note": "equal slices at once, each with its own phase origin: a timing, not the stream's bits"}}


def interpolated(x, D):
    """x -> D len(x) input-rate samples at f0 = 1 / D: zero-stuffed, D * a Blackman-windowed sinc of 32 taps a phase, phase by phase"""
    T = INTERP_TPP * D
    k = np.arange(T, dtype=np.float64)
    g = np.sinc((k - (T - 1) / 2.0) / D) * np.blackman(T)
    g *= D / g.sum()
    y = np.empty(len(x) * D, np.complex64)
    for p in range(D):
        y[p::D] = np.convolve(x, g[p::D].astype(np.float32))[: len(x)]
    rot = np.exp(2j * np.pi * (np.arange(D) / D)).astype(np.complex64)           # exp(2 pi i n / D) has the period D
    y.reshape(-1, D)[:] *= rot
    return y


def stream_block(n_fft, data_symbols, samples, reps, seed):
    D = STREAM_D
    probe = api.Context(n_fft=n_fft, modulation=api.QAM64, guard_bands=True)
    payload = data_symbols * probe.bytes_per_symbol - 16
    frame = probe.frame_samples(payload)
    rows = samples // (frame + 160) + 1
    c, pay, rx, Dsym = link(api.ECC_NONE, n_fft, api.QAM64, rows, payload, 30.0, seed)
    holdoff = frame - c.params.sync_window_reps * c.S
    x = api.pinned_empty((samples,), np.complex64); x[:] = rx.reshape(-1)[:samples].cpu().numpy()
    raw = api.pinned_empty((samples * D,), np.complex64); raw[:] = interpolated(x, D)
    inc = api.ddc_inc_for(1.0 / D)
    other = api.Context(n_fft=n_fft, modulation=api.QAM64, guard_bands=True)
    ref = other.decode_all_host(api.ddc_host(raw, D, inc), holdoff, 1 << 12, Dsym)
    ok = sum(int(ref["status"][k] == 0) for k in range(len(ref["status"])))
    out = {}
    rec = {"n_fft": n_fft, "narrow_samples": samples, "input_samples": samples * D, "decim": D, "taps": 24 * D, "frame_samples": frame,
           "packets_one_shot": int(len(ref["status"])), "packets_one_shot_ok": ok}

    def pushed(s, src, chunk, name):
        def f():
            s.reset()
            parts = [s.push_all(src[at: at + chunk], max_pkt=256) for at in range(0, len(src), chunk)]
            parts.append(s.flush(max_pkt=256))
            out[name] = {k: np.concatenate([p[k] for p in parts]) for k in ("bytes", "f_delta", "metric") + FIELDS}
        return f

    for chunk in CHUNKS:
        with c.stream(Dsym, holdoff, max_chunk=chunk // D) as plain, c.stream(Dsym, holdoff, max_chunk=chunk, ddc=(D, 1.0 / D, None)) as conv:
            ms = wall_alternated({"narrow_band": pushed(plain, x, chunk // D, "plain"), "converter_on": pushed(conv, raw, chunk, "conv")}, reps)
            assert same_packets(out["conv"], ref), f"the stream with the converter and the one-shot call on ddc_host(capture) differ at chunk {chunk}"
            pushes = (samples * D + chunk - 1) // chunk + 1
            r = {"pushes": pushes, "packets_narrow_band": int(len(out["plain"]["status"])), "packets_converter_on": int(len(out["conv"]["status"])),
                 "outputs_equal": True}
            for k, v in ms.items():
                r[k] = {**stat(v), "narrow_msamples_per_s": round(samples / stat(v)["ms_median"] / 1e3, 2), "ms_per_push": round(stat(v)["ms_median"] / pushes, 4)}
            r["ratio_on_over_narrow_band"] = round(r["converter_on"]["ms_median"] / r["narrow_band"]["ms_median"], 3)
            rec["chunk_%d" % chunk] = r
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", default="kernel_1Mi,kernel_16Mi,kernel_64Mi,host_16Mi,stream_n64,stream_n1024")
    ap.add_argument("--samples", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--f32-tflops", type=float, default=78.6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ddc_speed.json"))
    a = ap.parse_args()
    blocks = (("kernel_1Mi", lambda: kernel_block(1 << 20, a.reps, a.f32_tflops)), ("kernel_16Mi", lambda: kernel_block(1 << 24, a.reps, a.f32_tflops)),
              ("kernel_64Mi", lambda: kernel_block(1 << 26, a.reps, a.f32_tflops)), ("host_16Mi", lambda: host_block(1 << 24, a.host_threads)),
              ("stream_n64", lambda: stream_block(64, 29, a.samples, a.reps, 1201)), ("stream_n1024", lambda: stream_block(1024, 4, a.samples, a.reps, 1202)))
    rec, save = open_record({name: NOT_YET for name, _ in blocks}, a.out, keep_earlier=False)
    rec.update({"tool": "tools/bench_ddc.py", "device": torch.cuda.get_device_name(0), "reps": a.reps, "f32_tflops_assumed": a.f32_tflops,
                "method": "one process; one warm-up of every way, then alternated passes; kernel: the context's event timer around one push; "
                          "stream: wall clock around reset + every push + flush; median and spread (max - min)"})
    for name, f in blocks:
        if name in a.blocks.split(","):
            t0 = time.time()
            rec[name] = f()
            rec[name]["block_wall_s"] = round(time.time() - t0, 1)
            save()
            torch.cuda.empty_cache()
            print(name, "done in", rec[name]["block_wall_s"], "s", flush=True)


if __name__ == "__main__":
    main()
