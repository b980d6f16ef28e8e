"""Cost record of the FT4 soft-bit launch (cwslg_enable_ft4_softbits): stats.sync_ms per boundary with the feature off, on and off again --
same process, same box -- at 256 FT4 channels whose passbands carry synthetic FT4 transmissions (tests/ft4_softbits_ref.py), so that the
refinement hands out records.  Median over the measured boundaries after a warm-up; the two "off" legs bracket the "on" leg and give the
run-to-run spread the comparison is read against.  Also: sync records per channel and the added time per record.

    python scripts/ft4_softbits_cost.py [--channels 256] [--boundaries 7] [--out profiles/ft4_softbits_cost.json]
                                        [--parent-tree <checkout>]     # also: the parent commit's library, before and after, in child processes
    python scripts/ft4_softbits_cost.py --tree <other checkout> --off-only --out <file>     # e.g. the parent commit's library: the "off" leg alone
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--channels", type=int, default=256)
ap.add_argument("--boundaries", type=int, default=7, help="measured boundaries per leg (after --warmup)")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--max-cand", type=int, default=100)
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose package and library are measured")
ap.add_argument("--off-only", action="store_true", help="only the feature-off leg (a tree that does not have the feature)")
ap.add_argument("--parent-tree", default=None, help="checkout of the parent commit (built): its --off-only leg is run in a child process before and after")
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert args.channels >= 1 and args.boundaries >= 5
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tests"))
sys.path.insert(0, os.path.abspath(args.tree))
import cwsl_digi_amd as P                      # noqa: E402
from ft4_softbits_ref import ft4_iq_with_tones  # noqa: E402

FS, BLK = 48000, 1024
N = int(7.5 * FS) // BLK * BLK
rng = np.random.default_rng(1)
iq = (rng.normal(0.0, 30.0, N) + 1j * rng.normal(0.0, 30.0, N)).astype(np.complex64)
for k, rf in enumerate(np.arange(-23500.0, 23500.0, 450.0)):          # a transmission every 450 Hz: six or seven in every 3 kHz passband
    iq = iq + ft4_iq_with_tones(FS, N, rf, 0.0, 0.05 + 0.17 * (k % 9), 1500.0 + 250.0 * (k % 5), 100 + k)[0]
iq = iq.astype(np.complex64)



def parent_leg():
    """The --off-only leg of another checkout's library in a fresh process (this one holds no context meanwhile)."""
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "parent.json")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", args.parent_tree, "--off-only", "--channels", str(args.channels), "--boundaries",
                        str(args.boundaries), "--warmup", str(args.warmup), "--max-cand", str(args.max_cand), "--out", path], check=True, stdout=subprocess.DEVNULL)
        return json.load(open(path))["off"]


parent_before = parent_leg() if args.parent_tree else None
ctx = P.Context(0)
ctx.enable_sync(True, 1.5, args.max_cand, 200, 3000)
ctx.set_timing(True)
rx = ctx.receiver_open(FS, BLK, 0)
freqs = np.linspace(-FS // 2 + 100, FS // 2 - 6600, args.channels).astype(int)
chans = [ctx.channel_open(rx, int(f), "FT4") for f in freqs]
epoch = [10]
ctx.slot_boundary("FT4", epoch[0])


def _box():
    """What the figures were taken on: the device's name and compute-unit count as the runtime reports them."""
    import torch
    p = torch.cuda.get_device_properties(0)
    return dict(device=p.name, arch=getattr(p, "gcnArchName", ""), compute_units=p.multi_processor_count, hip=torch.version.hip)


def boundary():
    ctx.reset_stats()
    for k in range(0, N, 64 * BLK):
        ctx.push_iq(rx, iq[k:k + 64 * BLK])
    epoch[0] += 7
    ctx.slot_boundary("FT4", epoch[0])
    ctx.synchronize()
    s = ctx.stats()
    return s["sync_ms"], s["sync_launches"]


def leg(soft):
    if soft is not None:
        ctx.enable_ft4_softbits(soft)
    for _ in range(args.warmup):
        boundary()
    rows = [boundary() for _ in range(args.boundaries)]
    ms = sorted(r[0] for r in rows)
    return dict(sync_ms_median=float(np.median(ms)), sync_ms_min=ms[0], sync_ms_max=ms[-1], sync_ms=[round(r[0], 4) for r in rows],
                sync_launches_per_boundary=sorted(set(int(r[1]) for r in rows)))


out = dict(channels=args.channels, fs=FS, max_cand=args.max_cand, boundaries=args.boundaries, warmup=args.warmup,
           tree=os.path.basename(os.path.abspath(args.tree)), box=_box())
if args.off_only:
    out["off"] = leg(None)
else:
    out["off"] = leg(False)
    out["on"] = leg(True)
    n_rec, n_cand = [], []
    for ch in chans:                                                   # the lists of the last "on" boundary
        n_cand.append(len(ctx.fetch_candidates(ch, args.max_cand)))
        n_rec.append(len(ctx.fetch_ft4_sync(ch) or []))
    rec = ctx.fetch_ft4_softbits(chans[0])
    assert rec is not None and rec[0].shape[0] == n_rec[0]
    out["off_again"] = leg(False)
    assert ctx.fetch_ft4_softbits(chans[0]) is None
    total = int(sum(n_rec))
    added_ms = out["on"]["sync_ms_median"] - 0.5 * (out["off"]["sync_ms_median"] + out["off_again"]["sync_ms_median"])
    out.update(candidates_total=int(sum(n_cand)), records_total=total, records_per_channel_mean=total / args.channels,
               record_slots_launched=3 * args.max_cand * args.channels, added_sync_ms=added_ms,
               off_spread_ms=abs(out["off"]["sync_ms_median"] - out["off_again"]["sync_ms_median"]),
               added_us_per_record=1e3 * added_ms / max(total, 1))
ctx.close()
if parent_before is not None:
    out["parent_commit_same_box"] = dict(before=parent_before, after=parent_leg())
print(json.dumps(out))
path = args.out or os.path.join(HERE, "profiles", "ft4_softbits_cost.json")
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
with open(path, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
