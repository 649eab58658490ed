"""One pass of the A/B behind profiles/sc_margin_ab_parent.json: tools/bench_cfg3.py's config-3 data set (synth: 1 M slots, seed 3)
through the search alone (ctx.sc_correlate) and the chain over every lag (ctx.decode_batch), three timed blocks of ten steps each, with
the slow-list count and one sha256 over every output.

    python tools/lab/sc_margin_ab.py TREE OUT.json

TREE is the root of a built checkout (this one, or its parent with its own libofdm_hip.so): the script imports that tree's package and
tools.  Run the two trees alternately, one process a pass, five passes each, in one session on one GPU; the profile holds the ten
records and their medians."""
import hashlib
import json
import os
import sys

root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root)
os.chdir(root)
import torch  # noqa: E402

from ofdm_amd import api  # noqa: E402
from tools import bench_cfg3 as b3, rank_timing  # noqa: E402

import ofdm_amd  # noqa: E402
assert os.path.abspath(ofdm_amd.LIB_PATH).startswith(root), ofdm_amd.LIB_PATH
n_frames, steps = 1 << 20, 10
ctx = api.Context(n_fft=64, modulation=api.QAM64, guard_bands=True, device=0)
x, payload = b3.synth(api, torch, ctx, n_frames, seed=3)
D = ctx.data_symbols(b3.NBYTES)
out = {"tree": sys.argv[1], "frames": n_frames, "steps": steps}
for rep in range(3):   # three timed blocks of `steps` in the process; the first also warms up
    sms, _, sc = rank_timing.timed(ctx, torch, lambda: ctx.sc_correlate(x), steps)
    out.setdefault("search_ms", []).append(sms)
out["search_dispatch"] = ctx.last_dispatch()
out["slow_frames"] = ctx.get_tuning("stat_sc_slow_frames")
for rep in range(3):
    cms, _, res = rank_timing.timed(ctx, torch, lambda: ctx.decode_batch(x, max_symbols=D, n_lags=0), steps)
    out.setdefault("chain_ms", []).append(cms)
out["chain_dispatch"] = ctx.last_dispatch()
h = hashlib.sha256()
kept = res["bytes"][:, :b3.NBYTES] * (torch.arange(b3.NBYTES, device=ctx.device)[None, :] < res["len"][:, None])   # rows are defined up to len
for t in (sc[0], sc[1], sc[2], res["status"], res["offset"], res["len"], kept):
    h.update(t.cpu().numpy().tobytes())
out["outputs_sha256"] = h.hexdigest()
out["detections"] = int((sc[0] >= 0).sum())
os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
json.dump(out, open(sys.argv[2], "w"))
print(json.dumps(out))
