"""Cost record of the FT8 soft-bit launch (cwslg_enable_ft8_softbits): stats.sync_ms per boundary with the feature off, on and off again --
same process, same box -- at 1024 or more FT8 channels whose passbands carry synthetic transmissions (tests/ft8_signal.py), so that the
candidate lists are not empty.  Median over the measured boundaries after a warm-up; the two "off" legs bracket the "on" leg and give the
run-to-run spread the comparison is read against.  Also: candidates per channel and, from the lists themselves, the 128-byte lines a
candidate's 79 x 15 floats touch (the traffic estimate of DESIGN.md section 4) next to what the added time implies.

    python scripts/ft8_softbits_cost.py [--channels 1024] [--boundaries 7] [--out profiles/ft8_softbits_cost.json]
    python scripts/ft8_softbits_cost.py --tree <other checkout> --off-only      # e.g. the parent commit's library: the "off" leg alone
"""
import argparse
import json
import os
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--channels", type=int, default=1024)
ap.add_argument("--boundaries", type=int, default=7, help="measured boundaries per leg (after --warmup)")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--max-cand", type=int, default=200)
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose package and library are measured")
ap.add_argument("--off-only", action="store_true", help="only the feature-off leg (a tree that does not have the feature)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert args.channels >= 1024 and args.boundaries >= 5
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tests"))
sys.path.insert(0, os.path.abspath(args.tree))
import cwsl_digi_amd as P                      # noqa: E402
from ft8_signal import ft8_iq                  # noqa: E402

FS, BLK = 48000, 2048
N = 720000 // BLK * BLK
rng = np.random.default_rng(1)
iq = (rng.normal(0.0, 300.0, N) + 1j * rng.normal(0.0, 300.0, N)).astype(np.complex64)
for k, rf in enumerate(np.arange(-23500.0, 23500.0, 650.0)):          # a transmission every 650 Hz: four or five in every 3 kHz passband
    iq = iq + ft8_iq(FS, N, rf, 0.0, 0.1 + 0.23 * (k % 9), 1500.0 + 250.0 * (k % 5), rng)
iq = iq.astype(np.complex64)

ctx = P.Context(0)
ctx.enable_sync(True, 1.5, args.max_cand, 200, 3000)
ctx.set_timing(True)
rx = ctx.receiver_open(FS, BLK, 0)
freqs = np.linspace(-FS // 2 + 100, FS // 2 - 6600, args.channels).astype(int)
chans = [ctx.channel_open(rx, int(f), "FT8") for f in freqs]
epoch = [1]
ctx.slot_boundary("FT8", epoch[0])


def boundary():
    ctx.reset_stats()
    for k in range(0, N, 64 * BLK):
        ctx.push_iq(rx, iq[k:k + 64 * BLK])
    epoch[0] += 15
    ctx.slot_boundary("FT8", epoch[0])
    ctx.synchronize()
    s = ctx.stats()
    return s["sync_ms"], s["sync_spectra_ms"], s["sync_search_ms"], s["sync_launches"]


def leg(soft):
    if soft is not None:
        ctx.enable_ft8_softbits(soft)
    for _ in range(args.warmup):
        boundary()
    rows = [boundary() for _ in range(args.boundaries)]
    ms = sorted(r[0] for r in rows)
    return dict(sync_ms_median=float(np.median(ms)), sync_ms_min=ms[0], sync_ms_max=ms[-1], sync_ms=[round(r[0], 4) for r in rows],
                sync_spectra_ms_median=float(np.median([r[1] for r in rows])), sync_search_ms_median=float(np.median([r[2] for r in rows])),
                sync_launches_per_boundary=sorted(set(int(r[3]) for r in rows)))


out = dict(channels=args.channels, fs=FS, max_cand=args.max_cand, boundaries=args.boundaries, warmup=args.warmup, tree=os.path.basename(os.path.abspath(args.tree)))
if args.off_only:
    out["off"] = leg(None)
else:
    out["off"] = leg(False)
    out["on"] = leg(True)
    # the lists of the last "on" boundary: count, and the lines each candidate's rows touch (row pitch a multiple of 32 floats = one 128-byte line)
    n_cand, lines = [], 0
    for ch in chans:
        c = ctx.fetch_candidates(ch, args.max_cand)
        n_cand.append(len(c))
        for b, lag in ((x[0], x[1]) for x in c):
            m = lag + 12 + 4 * np.arange(79)
            rows_in = int(((m >= 1) & (m <= 372)).sum())
            lines += rows_in * (2 if b % 32 >= 18 else 1)
    rec = ctx.fetch_ft8_softbits(chans[0], args.max_cand)
    assert rec is not None and rec[0].shape[0] == n_cand[0]
    out["off_again"] = leg(False)
    total = int(sum(n_cand))
    added_ms = out["on"]["sync_ms_median"] - 0.5 * (out["off"]["sync_ms_median"] + out["off_again"]["sync_ms_median"])
    bytes_in = 128.0 * lines / max(total, 1)
    out.update(candidates_total=total, candidates_per_channel_mean=total / args.channels,
               estimate_bytes_per_candidate=dict(plane_lines=bytes_in, record=704, total=bytes_in + 704),
               added_sync_ms=added_ms, off_spread_ms=abs(out["off"]["sync_ms_median"] - out["off_again"]["sync_ms_median"]),
               added_us_per_candidate=1e3 * added_ms / max(total, 1),
               implied_gbytes_per_s=(bytes_in + 704) * total / max(added_ms, 1e-9) / 1e6)
print(json.dumps(out))
path = args.out or os.path.join(HERE, "profiles", "ft8_softbits_cost.json")
os.makedirs(os.path.dirname(path), exist_ok=True)
with open(path, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
ctx.close()
