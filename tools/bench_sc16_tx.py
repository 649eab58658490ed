#!/usr/bin/env python3
"""EXT-10 measurements: what sc16 (int16 I/Q) transmit output and sc16 long captures cost and save, one process on one MI355X ->
profiles/sc16_tx_speed.json.

Every comparison is taken in this one process; each side has `--reps` alternated passes (one warm-up of every variant, then rounds of all
of them in turn) and is reported as median and spread (max - min), in the style of tools/bench_sc16.py.  Blocks, saved one by one:

  fused    N = 64, 64-QAM, guard bands, 16 data symbols, 262 144 frames: k_txframe64_sc16 against the two-pass way a caller has without
           it (k_txframe64 + k_sc16_narrow, via no_txframe64_sc16) and against k_txframe64 alone (fc32 out).  The two sc16 variants
           write the SAME output buffer and their samples and counts are compared.  HBM bytes a sample: 4 / 20 / 8.
           Condition: fused faster than the two-pass path by more than the larger of the two spreads.
  host     encode_host_sc16 against encode_host into pinned memory, 65 536 frames, wall clock.
  long     decode_long_host_sc16 against decode_long_host on a 2 M-sample capture, pinned, wall clock.
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
from tools.link import alternated_ms, link, median, open_record  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak, as bench.py
SCALE = 30000.0        # 64-QAM with guard bands stays inside +-1: nothing clips


def stat(ms):
    return {"ms_all": [round(v, 5) for v in ms], "ms_median": round(median(ms), 5), "ms_spread": round(max(ms) - min(ms), 5)}


def wall_alternated(runs, reps):
    for f in runs.values():
        f()
    ms = {k: [] for k in runs}
    for _ in range(reps):
        for k, f in runs.items():
            t0 = time.perf_counter(); f(); ms[k].append((time.perf_counter() - t0) * 1e3)
    return ms


def fused(frames, reps):
    ctx = api.Context(n_fft=64, modulation=api.QAM64, guard_bands=True)
    two = api.Context(n_fft=64, modulation=api.QAM64, guard_bands=True, tuning={"no_txframe64_sc16": 1})
    nbytes = 16 * ctx.bytes_per_symbol - 16
    assert ctx.data_symbols(nbytes) == 16
    g = torch.Generator(device=ctx.device)
    g.manual_seed(101)
    pay = torch.randint(0, 256, (frames, nbytes), dtype=torch.uint8, device=ctx.device, generator=g)
    frame = ctx.frame_samples(nbytes)
    out16 = ctx.empty((frames, frame, 2), torch.int16)          # ONE sc16 output buffer, allocated after the input
    out32 = ctx.empty((frames, frame), torch.complex64)
    names, counts = {}, {}

    def run(name, c, f):
        def go():
            r = f()
            names[name] = c.last_dispatch()
            if isinstance(r, tuple):
                counts[name] = r[1]
        return c, go

    runs = {"sc16_fused": run("sc16_fused", ctx, lambda: ctx.encode_batch_sc16(pay, SCALE, out=out16, want_clipped=True)),
            "sc16_two_pass": run("sc16_two_pass", two, lambda: two.encode_batch_sc16(pay, SCALE, out=out16, want_clipped=True)),
            "fc32_k_txframe64": run("fc32_k_txframe64", ctx, lambda: ctx.encode_batch(pay, out=out32))}
    runs["sc16_fused"][1](); torch.cuda.synchronize()
    ref, ref_k = out16.clone(), counts["sc16_fused"].clone()
    runs["sc16_two_pass"][1](); torch.cuda.synchronize()
    same = bool(torch.equal(out16, ref)) and bool(torch.equal(counts["sc16_two_pass"], ref_k))
    clipped = int(ref_k.sum())
    del ref, ref_k
    ms = alternated_ms(runs, reps)
    n = frames * frame
    rec = {"frames": frames, "data_symbols": 16, "frame_samples": frame, "scale": SCALE, "clipped_components": clipped,
           "outputs_identical": same, "dispatch": names}
    for name, b in (("sc16_fused", 4), ("sc16_two_pass", 20), ("fc32_k_txframe64", 8)):
        m = median(ms[name])
        rec[name] = {**stat(ms[name]), "hbm_bytes_per_sample": b, "msamples_per_s": round(n / m / 1e3, 1),
                     "hbm_fraction": round(n * b / m / 1e6 / HBM_PEAK_GBS, 4)}
    f, t, c = (rec[k]["ms_median"] for k in ("sc16_fused", "sc16_two_pass", "fc32_k_txframe64"))
    rec["ratio_two_pass_over_fused"] = round(t / f, 4)
    rec["ratio_fc32_over_fused"] = round(c / f, 4)
    rec["condition_fused_faster_than_two_pass_by_more_than_the_larger_spread"] = bool(
        t - f > max(rec["sc16_fused"]["ms_spread"], rec["sc16_two_pass"]["ms_spread"]))
    return rec


def host(frames, reps):
    ctx = api.Context(n_fft=64, modulation=api.QAM64, guard_bands=True)
    nbytes = 16 * ctx.bytes_per_symbol - 16
    frame = ctx.frame_samples(nbytes)
    pay = np.random.default_rng(102).integers(0, 256, (frames, nbytes), dtype=np.uint8)
    o32 = api.pinned_empty((frames, frame), np.complex64)
    o16 = api.pinned_empty((frames, frame, 2), np.int16)
    ms = wall_alternated({"encode_host": lambda: ctx.encode_host(pay, out=o32),
                          "encode_host_sc16": lambda: ctx.encode_host_sc16(pay, SCALE, out=o16, want_clipped=True)}, reps)
    a, b = stat(ms["encode_host"]), stat(ms["encode_host_sc16"])
    want, _ = api.sc16_narrow(o32[:64], SCALE)
    return {"frames": frames, "fc32": {**a, "d2h_gbs": round(o32.nbytes / a["ms_median"] / 1e6, 2)},
            "sc16": {**b, "d2h_gbs": round(o16.nbytes / b["ms_median"] / 1e6, 2)},
            "first_64_frames_equal_the_narrowed_fc32_frames": bool(np.array_equal(o16[:64], want)),
            "ratio_fc32_over_sc16": round(a["ms_median"] / b["ms_median"], 4),
            "condition_sc16_faster_by_more_than_the_larger_spread": bool(a["ms_median"] - b["ms_median"] > max(a["ms_spread"], b["ms_spread"]))}


def long_capture(n, reps):
    c, pay, rx, D = link(api.ECC_NONE, 64, api.QAM64, 1, 400, 30.0, 103)
    rx = rx[0].cpu().numpy()
    rng = np.random.default_rng(103)
    sigma = 1e-3 * float(np.abs(rx).max())
    cap = (sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    at = (3 * n // 4) | 1
    cap[at: at + rx.size] += rx
    peak = float(max(np.abs(cap.real).max(), np.abs(cap.imag).max()))
    q, _ = api.sc16_narrow(cap, 0.9 * 32767.0 / peak)
    scale = float(np.float32(1.0) / np.float32(0.9 * 32767.0 / peak))
    x32 = api.pinned_empty((n,), np.complex64); x32[:] = api.sc16_widen(q, scale)
    x16 = api.pinned_empty((n, 2), np.int16); x16[:] = q
    res = {}
    ms = wall_alternated({"decode_long_host": lambda: res.__setitem__("fc32", c.decode_long_host(x32, D)),
                          "decode_long_host_sc16": lambda: res.__setitem__("sc16", c.decode_long_host_sc16(x16, D, scale=scale))}, reps)
    disp = c.last_dispatch()
    a, b = stat(ms["decode_long_host"]), stat(ms["decode_long_host_sc16"])
    same = all(res["fc32"][k] == res["sc16"][k] for k in ("status", "len", "offset", "f_delta", "metric")) and \
        bytes(res["fc32"]["bytes"][:400]) == bytes(res["sc16"]["bytes"][:400])
    return {"samples": n, "frame_at": at, "status": res["sc16"]["status"], "payload_delivered": bytes(res["sc16"]["bytes"][:400]) == bytes(pay[0].cpu().numpy()),
            "fc32": {**a, "h2d_gbs": round(x32.nbytes / a["ms_median"] / 1e6, 2)}, "sc16": {**b, "h2d_gbs": round(x16.nbytes / b["ms_median"] / 1e6, 2)},
            "sc16_dispatch": disp, "outputs_identical": bool(same), "ratio_fc32_over_sc16": round(a["ms_median"] / b["ms_median"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", default="fused,host,long")
    ap.add_argument("--frames", type=int, default=262144)
    ap.add_argument("--host-frames", type=int, default=65536)
    ap.add_argument("--long-samples", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sc16_tx_speed.json"))
    a = ap.parse_args()
    blocks = a.blocks.split(",")
    rec = {"tool": "tools/bench_sc16_tx.py", "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "method": "one process; per comparison one warm-up of every variant, then alternated passes; median and spread (max - min)"}
    rec, save = open_record(rec, a.out, keep_earlier=True)
    if "fused" in blocks:
        rec["fused"] = fused(a.frames, a.reps)
        save()
        torch.cuda.empty_cache()
    if "host" in blocks:
        rec["host"] = host(a.host_frames, a.reps)
        save()
    if "long" in blocks:
        rec["long_capture"] = long_capture(a.long_samples, a.reps)
        save()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
