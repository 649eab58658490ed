#!/usr/bin/env python3
"""EXT-15 measurements: the DC blocker (k_dc_block) alone and in front of a stream's window, one process on one MI355X
-> profiles/dcblock_speed.json.  No target is fixed in advance: the yardstick is the same build with the option off.

kernel   ofdm_dcblock_push / _push_sc16 of 1 Mi and of 16 Mi samples in ONE piece (max_chunk = the push), fc32 and sc16, M = 4 and 60,
         next to ofdm_hbm_read_probe (unit-stride 16-byte loads) over the bytes of the fc32 input; the context's event timer, every way
         alternated in this one process, `--reps` passes each after a warm-up, medians with spread (max - min).  The filter reads 8 (fc32) or
         4 (sc16) bytes a sample once from memory -- the halo and the second pass of a tile come from cache -- and writes 8.
stream   tools/bench_stream.py's two captures (`--samples` samples of tools/link.py's seeded link, 64-QAM with guard bands at 30 dB; N = 64
         and N = 1024) pushed through a stream in chunks of 4 Ki / 64 Ki / 1 Mi samples with the filter off and on (the default window),
         alternated, wall clock around reset + every push + flush.  Asserted in the same run: the stream with the filter delivers the
         packets of ONE decode_all_host call on dc_block_host(capture), every field bit for bit.
Whatever a call does not run stays "NOT YET MEASURED" in the record.
"""
import argparse
import json
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

CHUNKS = (4096, 65536, 1 << 20)
NOT_YET = "NOT YET MEASURED"


def kernel_block(n, reps):
    c = api.Context(n_fft=64, modulation=api.QAM64, guard_bands=True)
    g = torch.Generator(device="cpu").manual_seed(n % 1000)
    x = c.to_device((torch.randn(n, 2, generator=g) * 0.1 + 0.3).numpy().view(np.complex64).reshape(-1))
    q = c.to_device(torch.randint(-20000, 20000, (n, 2), generator=g, dtype=torch.int16).numpy())
    out = c.empty((n,), torch.complex64)
    probe = x[: n // 80 * 80]
    rec = {"samples": n, "hbm_read_probe_bytes": 8 * (n // 80 * 80)}
    filters = {M: c.dc_filter(M, max_chunk=n) for M in (4, 60)}
    runs = {"hbm_read_probe": (c, lambda: c.hbm_read_probe(probe, 2))}
    for M, f in filters.items():
        runs["fc32_M%d" % M] = (c, lambda f=f: f.push(x, out=out))
        runs["sc16_M%d" % M] = (c, lambda f=f: f.push(q, scale=1.0 / 32768, out=out))
    ms = alternated_ms(runs, reps)
    for k, v in ms.items():
        s = stat(v)
        nbytes = rec["hbm_read_probe_bytes"] if k == "hbm_read_probe" else (16 if k.startswith("fc32") else 12) * n
        rec[k] = {**s, "bytes_moved": nbytes, "gb_per_s": round(nbytes / s["ms_median"] / 1e6, 1)}
    filters[4].push(x, out=out)
    assert c.last_dispatch() == "k_dc_block<fc32>"
    for f in filters.values():
        f.close()
    return rec


def stream_block(n_fft, data_symbols, samples, reps, seed):
    probe = api.Context(n_fft=n_fft, modulation=api.QAM64, guard_bands=True)
    payload = data_symbols * probe.bytes_per_symbol - 16
    frame = probe.frame_samples(payload)
    rows = samples // (frame + 160) + 1
    c, pay, rx, D = link(api.ECC_NONE, n_fft, api.QAM64, rows, payload, 30.0, seed)
    holdoff = frame - c.params.sync_window_reps * c.S
    x = api.pinned_empty((samples,), np.complex64); x[:] = rx.reshape(-1)[:samples].cpu().numpy()
    M = api.dc_block_default(n_fft)
    other = api.Context(n_fft=n_fft, modulation=api.QAM64, guard_bands=True)
    ref = other.decode_all_host(api.dc_block_host(x, M), holdoff, 1 << 12, D)
    out = {}
    rec = {"n_fft": n_fft, "samples": samples, "frame_samples": frame, "dc_blocks": M}

    def pushed(s, chunk, name):
        def f():
            s.reset()
            parts = [s.push_all(x[at: at + chunk], max_pkt=256) for at in range(0, samples, chunk)]
            parts.append(s.flush(max_pkt=256))
            out[name] = {k: np.concatenate([p[k] for p in parts]) for k in ("bytes", "f_delta", "metric") + FIELDS}
        return f

    for chunk in CHUNKS:
        with c.stream(D, holdoff, max_chunk=chunk) as off, c.stream(D, holdoff, max_chunk=chunk, dc_blocks=M) as on:
            ms = wall_alternated({"filter_off": pushed(off, chunk, "off"), "filter_on": pushed(on, chunk, "on")}, reps)
            assert same_packets(out["on"], ref), f"the stream with the filter and the one-shot call on the filtered capture differ at chunk {chunk}"
            pushes = (samples + chunk - 1) // chunk + 1
            r = {"pushes": pushes, "packets_off": int(len(out["off"]["status"])), "packets_on": int(len(out["on"]["status"])), "outputs_equal": True}
            for k, v in ms.items():
                r[k] = {**stat(v), "msamples_per_s": round(samples / stat(v)["ms_median"] / 1e3, 2), "ms_per_push": round(stat(v)["ms_median"] / pushes, 4)}
            r["ratio_on_over_off"] = round(r["filter_on"]["ms_median"] / r["filter_off"]["ms_median"], 3)
            rec["chunk_%d" % chunk] = r
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", default="kernel_1Mi,kernel_16Mi,stream_n64,stream_n1024")
    ap.add_argument("--samples", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dcblock_speed.json"))
    a = ap.parse_args()
    rec = {"kernel_1Mi": NOT_YET, "kernel_16Mi": NOT_YET, "stream_n64": NOT_YET, "stream_n1024": NOT_YET}
    rec, save = open_record(rec, a.out, keep_earlier=False)
    rec.update({"tool": "tools/bench_dcblock.py", "device": torch.cuda.get_device_name(0), "reps": a.reps,
                "method": "one process; one warm-up of every way, then alternated passes; kernel: the context's event timer around one push; "
                          "stream: wall clock around reset + every push + flush; median and spread (max - min)"})
    todo = a.blocks.split(",")
    for name, f in (("kernel_1Mi", lambda: kernel_block(1 << 20, a.reps)), ("kernel_16Mi", lambda: kernel_block(1 << 24, a.reps)),
                    ("stream_n64", lambda: stream_block(64, 29, a.samples, a.reps, 1201)),
                    ("stream_n1024", lambda: stream_block(1024, 4, a.samples, a.reps, 1202))):
        if name in todo:
            t0 = time.time()
            rec[name] = f()
            rec[name]["block_wall_s"] = round(time.time() - t0, 1)
            save()
            torch.cuda.empty_cache()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
