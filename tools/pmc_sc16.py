"""Workload for one rocprofv3 --pmc pass over the EXT-9 kernels: k_demod64 on the widened samples and k_demod64_sc16 on the same int16
samples at the config-2 shape (262 144 frames of 16 symbols by default: beyond the 256 MiB Infinity Cache on both sides), then
k_sc16_widen and k_sc16_narrow.  Summarised by tools/pmc_summary.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from ofdm_amd import api  # noqa: E402
from tools.bench_sc16 import quantise_dev, synth_symbols  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 262144
ctx = api.Context(n_fft=64, modulation=api.QAM64, guard_bands=True)
x = synth_symbols(ctx, n, 16)
q, scale, _ = quantise_dev(ctx, x, 0.9)
ctx.sc16_widen(q, scale, out=x)
out = ctx.empty((n, 16 * ctx.bytes_per_symbol), torch.uint8)
q2 = torch.empty_like(q)
for _ in range(2):
    ctx.rx_demod(x, 16, out=out)
    ctx.rx_demod_sc16(q, 16, out=out, scale=scale)
    ctx.sc16_widen(q, scale, out=x)
    ctx.sc16_narrow(x, 1.0 / scale, out=q2)
torch.cuda.synchronize()
print("symbols", n * 16)
