#!/usr/bin/env python3
"""EXT-14 measurements: a capture pushed through a streaming receiver (ofdm_stream_push / ofdm_stream_push_sc16) chunk by chunk, against
ONE ofdm_rx_decode_all_long_host call on the same capture -- the parent commit's path and the baseline -- one process on one MI355X
-> profiles/stream_speed.json.

The captures are tools/bench_scan.py's: `--samples` samples (2 000 000) cut from the rows of tools/link.py's seeded link laid back to
back, 64-QAM with guard bands at 30 dB; N = 64 (29 data symbols: 3120-sample frames, about 600 of them) and N = 1024 (4 data symbols:
17 920-sample frames, about 110).  Both live in pinned host memory (the stream and the one-shot call DMA them in place), as fc32 and --
quantised to 0.9 of full scale -- as sc16.

Per block and chunk size (4 Ki, 64 Ki and 1 Mi samples), alternated in this one process with the one-shot call, `--reps` passes each
after one warm-up, wall clock: a pass is reset, every chunk pushed, flush.  Recorded: medians and spreads (max - min) of the pass,
sustained Msamples/s, time per push, packets delivered; asserted in the same run: the stream delivers the packets of the one-shot call
(of the widened capture, for sc16), every field bit for bit.

k_stream_ingest on its own, next to ofdm_hbm_read_probe (unit-stride 16-byte loads) over the same bytes, the context's event timer: a
stream with a holdoff of 2^39 samples whose first push commits a detection resumes its walk beyond every later lag, so every later push
is the H2D copy of the chunk and k_stream_ingest and nothing else (its dispatch string is asserted).  The copy alone (ofdm_memcpy_h2d of
the same bytes from the same pinned memory) is timed beside it; "ingest_minus_copy" is the difference of the two medians.
"""
import argparse
import ctypes as C
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
from tools.link import alternated_ms, link, open_record  # noqa: E402

CHUNKS = (4096, 65536, 1 << 20)
FIELDS = ("d1", "d_hat", "status", "len", "offset")


def same_packets(a, b):
    """every field of two result dicts, floats by their bits, bytes up to the delivered length"""
    if any(not np.array_equal(a[k], b[k]) for k in FIELDS):
        return False
    if not np.array_equal(a["f_delta"].view(np.int64), b["f_delta"].view(np.int64)) or not np.array_equal(a["metric"].view(np.int32), b["metric"].view(np.int32)):
        return False
    return all(int(a["status"][k]) != 0 or bytes(a["bytes"][k, : a["len"][k]]) == bytes(b["bytes"][k, : b["len"][k]]) for k in range(len(a["status"])))


def block(n_fft, data_symbols, samples, reps, seed):
    probe = api.Context(n_fft=n_fft, modulation=api.QAM64, guard_bands=True)
    payload = data_symbols * probe.bytes_per_symbol - 16
    frame = probe.frame_samples(payload)
    rows = samples // (frame + 160) + 1
    c, pay, rx, D = link(api.ECC_NONE, n_fft, api.QAM64, rows, payload, 30.0, seed)
    x_dev = rx.reshape(-1)[:samples].contiguous()
    holdoff = frame - c.params.sync_window_reps * c.S
    peak = float(torch.view_as_real(x_dev).abs().max())
    gain = float(np.float32(0.9 * 32767.0 / peak))
    q_dev, _ = c.sc16_narrow(x_dev, gain)
    scale = float(np.float32(1.0) / np.float32(gain))
    x = api.pinned_empty((samples,), np.complex64); x[:] = x_dev.cpu().numpy()
    q = api.pinned_empty((samples, 2), np.int16); q[:] = q_dev.cpu().numpy().reshape(samples, 2)
    xw = api.pinned_empty((samples,), np.complex64); xw[:] = api.sc16_widen(q, scale)
    other = api.Context(n_fft=n_fft, modulation=api.QAM64, guard_bands=True)
    out = {}
    rec = {"n_fft": n_fft, "samples": samples, "frame_samples": frame, "data_symbols": data_symbols, "holdoff": holdoff, "sc16_scale": scale,
           "horizon": c.params.sync_window_reps * c.S + (10 + D) * c.S + 2}

    def one_shot(src, name):
        def f():
            out[name] = other.decode_all_host(src, holdoff, 1 << 12, D)
        return f

    def pushed(s, src, chunk, name, sc16):
        def f():
            s.reset()
            parts = [s.push_all(src[at: at + chunk], sc16_scale=scale if sc16 else None, max_pkt=256) for at in range(0, samples, chunk)]
            parts.append(s.flush(max_pkt=256))
            out[name] = {k: np.concatenate([p[k] for p in parts]) for k in ("bytes", "f_delta", "metric") + FIELDS}
        return f

    for chunk in CHUNKS:
        with c.stream(D, holdoff, max_chunk=chunk) as s32, c.stream(D, holdoff, max_chunk=chunk) as s16:
            runs = {"one_shot_fc32": one_shot(x, "ref32"), "stream_fc32": pushed(s32, x, chunk, "s32", False),
                    "one_shot_of_widened": one_shot(xw, "ref16"), "stream_sc16": pushed(s16, q, chunk, "s16", True)}
            ms = wall_alternated(runs, reps)
            assert same_packets(out["s32"], out["ref32"]), f"fc32 stream and one-shot call differ at chunk {chunk}"
            assert same_packets(out["s16"], out["ref16"]), f"sc16 stream and one-shot call of the widened capture differ at chunk {chunk}"
            pushes = (samples + chunk - 1) // chunk + 1
            r = {"pushes": pushes, "packets": int(len(out["s32"]["status"])), "packets_sc16": int(len(out["s16"]["status"])), "outputs_equal": True}
            for k, v in ms.items():
                r[k] = {**stat(v), "msamples_per_s": round(samples / stat(v)["ms_median"] / 1e3, 2)}
            for k in ("stream_fc32", "stream_sc16"):
                r[k]["ms_per_push"] = round(r[k]["ms_median"] / pushes, 4)
            r["ratio_stream_fc32_over_one_shot"] = round(r["stream_fc32"]["ms_median"] / r["one_shot_fc32"]["ms_median"], 2)
            r["ratio_stream_sc16_over_one_shot"] = round(r["stream_sc16"]["ms_median"] / r["one_shot_of_widened"]["ms_median"], 2)
            rec["chunk_%d" % chunk] = r
    ok = out["ref32"]
    rec["payloads_delivered_exactly"] = sum(int(ok["status"][k] == 0 and ok["len"][k] == payload and bytes(ok["bytes"][k, :payload]) == bytes(pay[k].cpu().numpy()))
                                            for k in range(min(len(ok["status"]), pay.shape[0])))
    # k_stream_ingest alone: pushes of 1 Mi samples behind a committed detection under a holdoff no later lag reaches
    n1 = min(1 << 20, samples)
    far = 1 << 39
    with c.stream(D, far, max_chunk=n1) as s32, c.stream(D, far, max_chunk=n1) as s16:
        assert len(s32.push(x[:n1])["status"]) >= 1 and len(s16.push(q[:n1], sc16_scale=scale)["status"]) >= 1

        def copy(host, nbytes):
            return lambda: c._ck(c.lib.ofdm_memcpy_h2d(c.h, C.c_void_p(x_dev.data_ptr()), C.c_void_p(host.ctypes.data), nbytes), "h2d")

        keep = x_dev.clone()                                                    # (the copies land in x_dev: put it back afterwards)
        g = alternated_ms({"push_fc32": (c, lambda: s32.push(x[:n1], max_pkt=0)), "copy_fc32": (c, copy(x, 8 * n1)),
                           "push_sc16": (c, lambda: s16.push(q[:n1], max_pkt=0, sc16_scale=scale)), "copy_sc16": (c, copy(q, 4 * n1)),
                           "hbm_read_probe": (c, lambda: c.hbm_read_probe(keep[: n1 // 80 * 80], 2))}, reps)
        s32.push(x[:n1], max_pkt=0)
        d32 = c.last_dispatch()
        s16.push(q[:n1], max_pkt=0, sc16_scale=scale)
        d16 = c.last_dispatch()
        assert (d32, d16) == ("k_stream_ingest<fc32>", "k_stream_ingest<sc16>"), (d32, d16)
        x_dev.copy_(keep)
    st = {k: stat(v) for k, v in g.items()}
    rec["ingest_alone_1Mi"] = {
        **st, "samples": n1,
        "fc32": {"bytes_read": 8 * n1, "bytes_written": 8 * n1, "ingest_minus_copy_ms": round(st["push_fc32"]["ms_median"] - st["copy_fc32"]["ms_median"], 4)},
        "sc16": {"bytes_read": 4 * n1, "bytes_written": 8 * n1, "ingest_minus_copy_ms": round(st["push_sc16"]["ms_median"] - st["copy_sc16"]["ms_median"], 4)},
        "hbm_read_probe_bytes": 8 * (n1 // 80 * 80),
        "note": "push_*: H2D copy of the chunk from pinned memory + k_stream_ingest (nothing kept: the whole launch moves the chunk); copy_*: the "
                "same bytes through ofdm_memcpy_h2d alone"}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", default="n64,n1024")
    ap.add_argument("--samples", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_speed.json"))
    a = ap.parse_args()
    rec = {"tool": "tools/bench_stream.py", "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "method": "one process; one warm-up of every way, then alternated passes; wall clock around reset + every push + flush and around "
                     "the one-shot call; median and spread (max - min)"}
    rec, save = open_record(rec, a.out, keep_earlier=True)
    for name, n_fft, syms, seed in (("n64", 64, 29, 1201), ("n1024", 1024, 4, 1202)):
        if name in a.blocks.split(","):
            t0 = time.time()
            rec[name] = block(n_fft, syms, a.samples, a.reps, seed)
            rec[name]["block_wall_s"] = round(time.time() - t0, 1)
            save()
            torch.cuda.empty_cache()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
