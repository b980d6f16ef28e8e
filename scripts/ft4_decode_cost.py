"""Cost record of the FT4 decode launch (cwslg_enable_ft4_decode): stats.sync_ms per boundary with FT4 soft bits on and the decode off, on and off
again -- same process, same box -- on the workload of scripts/ft4_softbits_cost.py: 256 FT4 channels at 48 kHz whose passbands carry synthetic FT4
transmissions (tests/ft4_softbits_ref.py), so that the refinement hands out records.  Median over the measured boundaries after a warm-up; the
two "off" legs bracket the "on" leg.  The code is one of the test codes (tests/ldpc_cases.py) and the transmissions carry random tones, not
codewords: what is timed is the decoder's work on records that do NOT decode -- the bulk of any real list -- and the shares below say how much
of it there was.  With --parent-tree this process opens no context itself: it runs three child processes in a row -- the parent commit's library
(soft bits on, no decode), this tree's three legs, the parent's again -- and records them together; "off costs nothing" is read as: both off-leg medians lie inside the parent's own boundary
spread on that box.

    python scripts/ft4_decode_cost.py [--channels 256] [--boundaries 7] [--out profiles/ft4_decode_cost.json]
                                      [--parent-tree <checkout>]      # also: the parent commit's library, before and after, in child processes
    python scripts/ft4_decode_cost.py --tree <other checkout> --off-only --out <file>     # e.g. the parent commit's library: the "off" leg alone
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
ap.add_argument("--max-iter", type=int, default=30)
ap.add_argument("--min-nsync", type=int, default=8)
ap.add_argument("--min-nqual", type=int, default=20)
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose package and library are measured")
ap.add_argument("--off-only", action="store_true", help="only the decode-off leg (a tree that does not have the feature)")
ap.add_argument("--parent-tree", default=None, help="checkout of the parent commit (built): its --off-only leg is run in a child process before and after")
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert args.channels >= 1 and args.boundaries >= 5
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def finish(out):
    print(json.dumps(out))
    path = args.out or os.path.join(HERE, "profiles", "ft4_decode_cost.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


def child(tree, off_only):
    """One run of this script in a fresh process: another checkout's --off-only leg, or this tree's three legs."""
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "run.json")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", tree, "--channels", str(args.channels), "--boundaries", str(args.boundaries),
                        "--warmup", str(args.warmup), "--max-cand", str(args.max_cand), "--max-iter", str(args.max_iter), "--min-nsync", str(args.min_nsync),
                        "--min-nqual", str(args.min_nqual), "--out", path] + (["--off-only"] if off_only else []), check=True, stdout=subprocess.DEVNULL)
        return json.load(open(path))


if args.parent_tree:
    before = child(args.parent_tree, True)["off"]
    out = child(args.tree, args.off_only)
    parents = dict(before=before, after=child(args.parent_tree, True)["off"])
    lo = min(p["sync_ms_min"] for p in parents.values())
    hi = max(p["sync_ms_max"] for p in parents.values())
    out.update(parent_commit_same_box=parents, parent_sync_ms_medians=[parents["before"]["sync_ms_median"], parents["after"]["sync_ms_median"]],
               parent_sync_ms_range=[lo, hi])
    if "off_again" in out:
        out["off_inside_parent_range"] = bool(all(lo <= o["sync_ms_median"] <= hi for o in (out["off"], out["off_again"])))
    finish(out)
    sys.exit(0)

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


ctx = P.Context(0)
ctx.enable_sync(True, 1.5, args.max_cand, 200, 3000)
ctx.enable_ft4_softbits(True)
ctx.set_timing(True)
if not args.off_only:
    import ldpc_cases                          # noqa: E402
    ctx.set_ldpc_code(ldpc_cases.make_code(ldpc_cases.SEEDS[0])["nm"])
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


def leg(decode):
    if decode is not None:
        ctx.enable_ft4_decode(decode, args.max_iter, args.min_nsync, args.min_nqual)
    for _ in range(args.warmup):
        boundary()
    rows = [boundary() for _ in range(args.boundaries)]
    ms = sorted(r[0] for r in rows)
    return dict(sync_ms_median=float(np.median(ms)), sync_ms_min=ms[0], sync_ms_max=ms[-1], sync_ms_spread=ms[-1] - ms[0], sync_ms=[round(r[0], 4) for r in rows],
                sync_launches_per_boundary=sorted(set(int(r[1]) for r in rows)))


out = dict(channels=args.channels, fs=FS, max_cand=args.max_cand, boundaries=args.boundaries, warmup=args.warmup, soft_bits="on in every leg",
           tree=os.path.basename(os.path.abspath(args.tree)), box=_box())
if args.off_only:
    out["off"] = leg(None)
else:
    out.update(max_iter=args.max_iter, min_nsync=args.min_nsync, min_nqual=args.min_nqual)
    out["off"] = leg(False)
    out["on"] = leg(True)
    records = gated_in = sets = attempted = iters = crc_ok = 0
    for ch in chans:                                                   # the records of the last "on" boundary
        rec = ctx.fetch_ft4_decode(ch)
        assert rec is not None and len(rec) == len(ctx.fetch_ft4_sync(ch) or [])
        it = rec["set"]["iters"]
        att = it >= 0
        records += len(rec); gated_in += int(att.any(axis=1).sum()); sets += att.size; attempted += int(att.sum()); iters += int(it[att].sum())
        crc_ok += int(rec["set"]["crc_ok"].sum())
    out["off_again"] = leg(False)
    assert ctx.fetch_ft4_decode(chans[0]) is None
    offs = (out["off"], out["off_again"])
    added_ms = out["on"]["sync_ms_median"] - 0.5 * (offs[0]["sync_ms_median"] + offs[1]["sync_ms_median"])
    out.update(records_total=records, records_per_channel_mean=records / args.channels, records_attempted=gated_in,
               records_attempted_share=gated_in / max(records, 1), sets_total=sets, sets_attempted=attempted, sets_attempted_share=attempted / max(sets, 1),
               iterations_per_attempted_set_mean=iters / max(attempted, 1), sets_crc_ok=crc_ok,
               waves_launched=9 * args.max_cand * args.channels, added_sync_ms=added_ms,
               off_spread_within_ms=[o["sync_ms_spread"] for o in offs],
               off_spread_between_ms=abs(offs[0]["sync_ms_median"] - offs[1]["sync_ms_median"]),
               added_us_per_record=1e3 * added_ms / max(records, 1), added_us_per_attempted_set=1e3 * added_ms / max(attempted, 1),
               added_ns_per_attempted_iteration=1e6 * added_ms / max(iters, 1))
ctx.close()
finish(out)
