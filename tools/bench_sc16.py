#!/usr/bin/env python3
"""EXT-9 measurements: what sc16 (int16 I/Q) input costs and saves, one process on one MI355X -> profiles/sc16_speed.json.

Every comparison is taken in this one process; each side has `--reps` alternated passes (tools/link.py alternated_ms: one warm-up of
every variant, then rounds of all of them in turn) and is reported as median and spread (max - min).  Blocks, saved one by one:

  cfg2     the headline shape (N = 64, 64-QAM, guard bands, frames of 16 symbols): k_demod64 on the widened samples, k_demod64_sc16,
           and the sc16 call under no_demod64_sc16 (k_sc16_widen + k_demod64).  All three write into the SAME output buffer, allocated
           after the inputs, and their bytes are compared.  Condition: fused faster than the widen path by more than the larger spread.
           The ratio against fc32 has no threshold (ceiling about 1.5x from the bytes: 548 -> at most 356 per symbol).
  stages   k_sc16_widen and k_sc16_narrow (12 bytes a sample each) next to ofdm_hbm_read_probe pattern 2 on the fc32 buffer.
  host     demod_host against demod_host_sc16 and decode_host against decode_host_sc16, pinned input, tools/bench_host.py's sizes, wall
           clock.  Condition: each sc16 pass faster than its fc32 pass by more than the larger spread.
  chain    decode_batch against decode_batch_sc16, device-resident, 65 536 N = 64 frames: the cost of the widen pass.
  quant    LDPC648 at N = 64 on the 6 dB link (tools/link.py, the README table's shape): frames right / wrong / reported for the fc32
           capture and for the same capture through sc16 at 0.9 and at 1/16 of full scale.  An observation: no threshold.
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
from tools.link import alternated_ms, delivered, link, median, open_record  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak, as bench.py


def stat(ms):
    return {"ms_all": [round(v, 5) for v in ms], "ms_median": round(median(ms), 5), "ms_spread": round(max(ms) - min(ms), 5)}


def quantise_dev(ctx, x, peak_fraction):
    """complex64 [F, L] on the device -> (int16 [F, L, 2], scale): the largest component at peak_fraction of full scale"""
    peak = float(torch.view_as_real(x).abs().max())
    gain = float(np.float32(peak_fraction * 32767.0 / peak))
    q, clipped = ctx.sc16_narrow(x, gain)
    return q, float(np.float32(1.0) / np.float32(gain)), int(clipped.sum())


def synth_symbols(ctx, frames, syms, seed=77):
    """[frames, syms * S] symbols of the library's TX path plus 30 dB noise, in chunks"""
    g = torch.Generator(device=ctx.device)
    g.manual_seed(seed)
    x = torch.empty((frames, syms * ctx.S), dtype=torch.complex64, device=ctx.device)
    chunk = 65536
    for lo in range(0, frames, chunk):
        hi = min(lo + chunk, frames)
        pay = torch.randint(0, 256, ((hi - lo) * syms * ctx.bytes_per_symbol,), dtype=torch.uint8, device=ctx.device, generator=g)
        blk = ctx.tx_symbols(pay).view(hi - lo, syms * ctx.S)
        sigma = float(blk.abs().pow(2).mean().sqrt()) * 10 ** (-30.0 / 20) / np.sqrt(2.0)
        nz = torch.randn((hi - lo, syms * ctx.S, 2), dtype=torch.float32, device=ctx.device, generator=g) * sigma
        x[lo:hi] = blk + torch.view_as_complex(nz)
        del blk, nz, pay
    return x


def cfg2(frames, syms, reps):
    ctx = api.Context(n_fft=64, modulation=api.QAM64, guard_bands=True)
    wid = api.Context(n_fft=64, modulation=api.QAM64, guard_bands=True, tuning={"no_demod64_sc16": 1})
    x = synth_symbols(ctx, frames, syms)
    q, scale, clipped = quantise_dev(ctx, x, 0.9)
    ctx.sc16_widen(q, scale, out=x)                         # the fc32 twin: exactly the widened samples
    out = ctx.empty((frames, syms * ctx.bytes_per_symbol), torch.uint8)   # ONE output buffer, allocated after the inputs
    names = {}

    def run(name, c, f):
        def go():
            f()
            names[name] = c.last_dispatch()
        return c, go

    runs = {"fc32_k_demod64": run("fc32_k_demod64", ctx, lambda: ctx.rx_demod(x, syms, out=out)),
            "sc16_fused": run("sc16_fused", ctx, lambda: ctx.rx_demod_sc16(q, syms, out=out, scale=scale)),
            "sc16_widen_path": run("sc16_widen_path", wid, lambda: wid.rx_demod_sc16(q, syms, out=out, scale=scale))}
    ref = None
    same = True
    for name, (c, go) in runs.items():
        go(); torch.cuda.synchronize()
        if ref is None:
            ref = out.clone()
        else:
            same = same and bool(torch.equal(out, ref))
    del ref
    ms = alternated_ms(runs, reps)
    n_sym = frames * syms
    rec = {"frames": frames, "syms_per_frame": syms, "scale": scale, "clipped_by_the_quantiser": clipped, "outputs_identical": same,
           "dispatch": names}
    for name in runs:
        rec[name] = stat(ms[name])
    f, s, w = (rec[k]["ms_median"] for k in ("fc32_k_demod64", "sc16_fused", "sc16_widen_path"))
    out_b = ctx.bytes_per_symbol
    rec["fc32_k_demod64"]["hbm_fraction_fetched_512_plus_out"] = round(n_sym * (512 + out_b) / f / 1e6 / HBM_PEAK_GBS, 4)
    rec["sc16_fused"]["hbm_fraction_fetched_320_plus_out"] = round(n_sym * (320 + out_b) / s / 1e6 / HBM_PEAK_GBS, 4)
    rec["sc16_fused"]["hbm_fraction_data_256_plus_out"] = round(n_sym * (256 + out_b) / s / 1e6 / HBM_PEAK_GBS, 4)
    rec["sc16_fused"]["msamples_per_s"] = round(n_sym * ctx.S / s / 1e3, 1)
    rec["fc32_k_demod64"]["msamples_per_s"] = round(n_sym * ctx.S / f / 1e3, 1)
    rec["ratio_fc32_over_fused"] = round(f / s, 4)
    rec["ratio_widen_path_over_fused"] = round(w / s, 4)
    rec["condition_fused_faster_than_widen_path_by_more_than_the_larger_spread"] = bool(
        w - s > max(rec["sc16_fused"]["ms_spread"], rec["sc16_widen_path"]["ms_spread"]))
    return rec, (ctx, x, q, scale)


def stages(ctx, x, q, scale, reps):
    q2 = torch.empty_like(q)
    gain = float(np.float32(1.0) / np.float32(scale))
    runs = {"hbm_read_probe_pattern2": (ctx, lambda: ctx.hbm_read_probe(x, 2)),
            "k_sc16_widen": (ctx, lambda: ctx.sc16_widen(q, scale, out=x)),
            "k_sc16_narrow": (ctx, lambda: ctx.sc16_narrow(x, gain, out=q2))}
    ms = alternated_ms(runs, reps)
    n = x.numel()
    rec = {"samples": n, "narrow_inverts_widen": bool(torch.equal(q2, q))}
    for name, b in (("hbm_read_probe_pattern2", 8), ("k_sc16_widen", 12), ("k_sc16_narrow", 12)):
        rec[name] = {**stat(ms[name]), "bytes_per_sample": b, "gbs": round(n * b / median(ms[name]) / 1e6, 1),
                     "hbm_fraction": round(n * b / median(ms[name]) / 1e6 / HBM_PEAK_GBS, 4)}
    return rec


def wall_alternated(runs, reps):
    for f in runs.values():
        f()
    ms = {k: [] for k in runs}
    for _ in range(reps):
        for k, f in runs.items():
            t0 = time.perf_counter(); f(); ms[k].append((time.perf_counter() - t0) * 1e3)
    return ms


def host_and_chain(frames2, frames3, reps):
    from tools import bench_cfg3

    ctx = api.Context(n_fft=64, modulation=api.QAM64, guard_bands=True)
    rec = {}
    # config-2 shape through the host pipe
    syms = 16
    x_dev = synth_symbols(ctx, frames2, syms)
    q_dev, scale, _ = quantise_dev(ctx, x_dev, 0.9)
    ctx.sc16_widen(q_dev, scale, out=x_dev)
    x = api.pinned_empty(tuple(x_dev.shape), np.complex64); x[:] = x_dev.cpu().numpy()
    q = api.pinned_empty(tuple(q_dev.shape), np.int16); q[:] = q_dev.cpu().numpy()
    res = api.pinned_empty((frames2, syms * ctx.bytes_per_symbol), np.uint8)
    res2 = api.pinned_empty((frames2, syms * ctx.bytes_per_symbol), np.uint8)
    ms = wall_alternated({"demod_host": lambda: ctx.demod_host(x, syms, out=res),
                          "demod_host_sc16": lambda: ctx.demod_host_sc16(q, syms, out=res2, scale=scale)}, reps)
    a, b = stat(ms["demod_host"]), stat(ms["demod_host_sc16"])
    rec["demod_host"] = {"frames": frames2, "fc32": {**a, "h2d_gbs": round(x.nbytes / a["ms_median"] / 1e6, 2)},
                         "sc16": {**b, "h2d_gbs": round(q.nbytes / b["ms_median"] / 1e6, 2)}, "outputs_identical": bool(np.array_equal(res, res2)),
                         "ratio_fc32_over_sc16": round(a["ms_median"] / b["ms_median"], 4),
                         "condition_sc16_faster_by_more_than_the_larger_spread": bool(a["ms_median"] - b["ms_median"] > max(a["ms_spread"], b["ms_spread"]))}
    del x_dev, q_dev, x, q
    # config-3 shape: the whole chain, through the host pipe and device-resident
    caps_dev, _ = bench_cfg3.synth(api, torch, ctx, frames3, seed=11)
    D = ctx.data_symbols(bench_cfg3.NBYTES)
    qc_dev, scale, _ = quantise_dev(ctx, caps_dev, 0.9)
    ctx.sc16_widen(qc_dev, scale, out=caps_dev)
    caps = api.pinned_empty(tuple(caps_dev.shape), np.complex64); caps[:] = caps_dev.cpu().numpy()
    qc = api.pinned_empty(tuple(qc_dev.shape), np.int16); qc[:] = qc_dev.cpu().numpy()
    got = ctx.decode_host(caps, max_symbols=D)
    got2 = ctx.decode_host_sc16(qc, max_symbols=D, scale=scale)
    same = all(np.array_equal(got[k], got2[k]) for k in got)
    ms = wall_alternated({"decode_host": lambda: ctx.decode_host(caps, max_symbols=D, out=got),
                          "decode_host_sc16": lambda: ctx.decode_host_sc16(qc, max_symbols=D, out=got2, scale=scale)}, reps)
    a, b = stat(ms["decode_host"]), stat(ms["decode_host_sc16"])
    rec["decode_host"] = {"frames": frames3, "fc32": {**a, "h2d_gbs": round(caps.nbytes / a["ms_median"] / 1e6, 2)},
                          "sc16": {**b, "h2d_gbs": round(qc.nbytes / b["ms_median"] / 1e6, 2)}, "outputs_identical": bool(same),
                          "frames_ok": int((got["status"] == 0).sum()), "ratio_fc32_over_sc16": round(a["ms_median"] / b["ms_median"], 4),
                          "condition_sc16_faster_by_more_than_the_larger_spread": bool(a["ms_median"] - b["ms_median"] > max(a["ms_spread"], b["ms_spread"]))}
    msd = alternated_ms({"decode_batch": (ctx, lambda: ctx.decode_batch(caps_dev, max_symbols=D)),
                         "decode_batch_sc16": (ctx, lambda: ctx.decode_batch_sc16(qc_dev, max_symbols=D, scale=scale))}, reps)
    disp = ctx.last_dispatch()
    a, b = stat(msd["decode_batch"]), stat(msd["decode_batch_sc16"])
    rec["chain_device_resident"] = {"frames": frames3, "fc32": a, "sc16": b, "sc16_dispatch": disp,
                                    "widen_pass_costs_ms": round(b["ms_median"] - a["ms_median"], 5),
                                    "ratio_sc16_over_fc32": round(b["ms_median"] / a["ms_median"], 4)}
    return rec


def quant(n_frames=4096, payload=560, snr=6.0, seed=11):
    c, pay, rx, D = link(api.ECC_LDPC648, 64, api.QAM64, n_frames, payload, snr, seed)
    out = {"snr_db": snr, "frames": n_frames, "payload": payload, "seed": seed, "ecc": "LDPC648", "n_fft": 64}

    def count(r):
        right, ok = delivered(r, pay, payload)
        return {"right": int(right.sum()), "wrong": int((ok & ~right).sum()), "reported": int((~ok).sum())}

    out["fc32"] = count(c.decode_batch(rx, max_symbols=D))
    for name, frac in (("sc16_at_0.9_of_full_scale", 0.9), ("sc16_at_1/16_of_full_scale", 1.0 / 16)):
        q, scale, clipped = quantise_dev(c, rx, frac)
        out[name] = {**count(c.decode_batch_sc16(q, max_symbols=D, scale=scale)), "clipped_components": clipped,
                     "peak_int16": int(q.to(torch.int32).abs().max())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", default="cfg2,stages,host,chain,quant")
    ap.add_argument("--frames", type=int, default=1_000_000, help="cfg2: frames of 16 symbols (BASELINE config 2: 1 M)")
    ap.add_argument("--host-frames2", type=int, default=131072)
    ap.add_argument("--host-frames3", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sc16_speed.json"))
    a = ap.parse_args()
    blocks = a.blocks.split(",")
    rec = {"tool": "tools/bench_sc16.py", "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "method": "one process; per comparison one warm-up of every variant, then alternated passes; median and spread (max - min)"}
    rec, save = open_record(rec, a.out, keep_earlier=True)
    if "cfg2" in blocks or "stages" in blocks:
        r, (ctx, x, q, scale) = cfg2(a.frames, 16, a.reps)
        rec["cfg2"] = r
        save()
        if "stages" in blocks:
            rec["stages"] = stages(ctx, x, q, scale, a.reps)
            save()
        del ctx, x, q
        torch.cuda.empty_cache()
    if "host" in blocks or "chain" in blocks:
        rec.update(host_and_chain(a.host_frames2, a.host_frames3, a.reps))
        save()
    if "quant" in blocks:
        rec["quantisation"] = quant()
        save()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
