"""Cost record of the FT4 OSD launch (cwslg_enable_ft4_osd): stats.sync_ms per boundary with FT4 soft bits and the FT4 decode on in every leg and OSD
off, on at order 1, on at order 2 and off again -- same process, same box -- on the workload of scripts/ft4_decode_cost.py: 256 FT4 channels at
48 kHz whose passbands carry synthetic FT4 transmissions (tests/ft4_softbits_ref.py) with random tones, not codewords, so every attempted set
fails belief propagation and goes on to OSD: the bulk of any real list.  Median over the measured boundaries after a warm-up; the two "off" legs
bracket the "on" legs.  The code is one of the test codes (tests/ldpc_cases.py).  Per "on" leg the record says how many sets were attempted and
how many the record-level gate spared (sets BP left without crc_ok in a record another set of which BP decoded).  With --parent-tree this
process opens no context itself: it runs three child processes in a row -- the parent commit's library (soft bits and decode on, no OSD), this
tree's four legs, the parent's again -- and records them together; "off costs nothing" is read as: both off-leg medians lie inside the parent's
own boundary spread on that box.

    python scripts/ft4_osd_cost.py [--channels 256] [--boundaries 7] [--out profiles/ft4_osd_cost.json]
                                   [--parent-tree <checkout>]      # also: the parent commit's library, before and after, in child processes
    python scripts/ft4_osd_cost.py --tree <other checkout> --off-only --out <file>     # e.g. the parent commit's library: the "off" leg alone
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
ap.add_argument("--off-only", action="store_true", help="only the OSD-off leg (a tree that does not have the feature)")
ap.add_argument("--parent-tree", default=None, help="checkout of the parent commit (built): its --off-only leg is run in a child process before and after")
ap.add_argument("--child-timeout", type=float, default=240.0, help="seconds one child process may take: a child that hangs must not hold the card")
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert args.channels >= 1 and args.boundaries >= 5
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def finish(out):
    print(json.dumps(out))
    path = args.out or os.path.join(HERE, "profiles", "ft4_osd_cost.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


def child(tree, off_only):
    """One run of this script in a fresh process: another checkout's --off-only leg, or this tree's four legs."""
    print("child: %s%s" % (os.path.basename(os.path.abspath(tree)), " (off only)" if off_only else ""), file=sys.stderr, flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "run.json")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", tree, "--channels", str(args.channels), "--boundaries", str(args.boundaries),
                        "--warmup", str(args.warmup), "--max-cand", str(args.max_cand), "--max-iter", str(args.max_iter), "--min-nsync", str(args.min_nsync),
                        "--min-nqual", str(args.min_nqual), "--out", path] + (["--off-only"] if off_only else []), check=True, stdout=subprocess.DEVNULL,
                       timeout=args.child_timeout)
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
import ldpc_cases                              # noqa: E402
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
ctx.set_ldpc_code(ldpc_cases.make_code(ldpc_cases.SEEDS[0])["nm"])
ctx.enable_ft4_decode(True, args.max_iter, args.min_nsync, args.min_nqual)
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


def leg(order):
    """order None: leave the context as it is (a tree without the feature); -1: OSD off; 0..2: on."""
    if order is not None:
        ctx.enable_ft4_osd(order >= 0, max(order, 0), args.min_nsync, args.min_nqual)
    for _ in range(args.warmup):
        boundary()
    rows = [boundary() for _ in range(args.boundaries)]
    ms = sorted(r[0] for r in rows)
    out = dict(sync_ms_median=float(np.median(ms)), sync_ms_min=ms[0], sync_ms_max=ms[-1], sync_ms_spread=ms[-1] - ms[0], sync_ms=[round(r[0], 4) for r in rows],
               sync_launches_per_boundary=sorted(set(int(r[1]) for r in rows)))
    if order is not None and order >= 0:                               # the records of the leg's last boundary
        records = sets = attempted = spared = bp_records = crc_ok = 0
        hows = np.zeros(3, int)
        for ch in chans:
            rec, msg = ctx.fetch_ft4_osd(ch), ctx.fetch_ft4_decode(ch)
            assert rec is not None and msg is not None and len(rec) == len(msg) == len(ctx.fetch_ft4_sync(ch) or [])
            att = rec["set"]["how"] != 0xff
            bp = msg["set"]["crc_ok"] != 0
            # what a per-set gate would have attempted and the record gate does not: the failed sets of a record BP decoded in another set
            spared += int(((msg["set"]["iters"] >= 0) & ~bp & bp.any(axis=1)[:, None]).sum())
            records += len(rec); sets += att.size; attempted += int(att.sum()); bp_records += int(bp.any(axis=1).sum())
            crc_ok += int(rec["set"]["crc_ok"].sum())
            hows += np.bincount(rec["set"]["how"][att], minlength=3)[:3]
        out.update(records_total=records, sets_total=sets, sets_attempted=attempted, sets_attempted_share=attempted / max(sets, 1),
                   records_decoded_by_bp=bp_records, sets_spared_by_the_record_gate=spared, sets_crc_ok=crc_ok, winners_by_flips=[int(h) for h in hows],
                   waves_launched=9 * args.max_cand * args.channels)
    return out


out = dict(channels=args.channels, fs=FS, max_cand=args.max_cand, boundaries=args.boundaries, warmup=args.warmup, soft_bits_and_decode="on in every leg",
           max_iter=args.max_iter, min_nsync=args.min_nsync, min_nqual=args.min_nqual, tree=os.path.basename(os.path.abspath(args.tree)), box=_box())
if args.off_only:
    out["off"] = leg(None)
else:
    out["off"] = leg(-1)
    out["order1"] = leg(1)
    out["order2"] = leg(2)
    out["off_again"] = leg(-1)
    assert ctx.fetch_ft4_osd(chans[0]) is None
    offs = (out["off"], out["off_again"])
    base = 0.5 * (offs[0]["sync_ms_median"] + offs[1]["sync_ms_median"])
    for name in ("order1", "order2"):
        o = out[name]
        o["added_sync_ms"] = o["sync_ms_median"] - base
        o["added_us_per_attempted_set"] = 1e3 * o["added_sync_ms"] / max(o["sets_attempted"], 1)
    out.update(off_spread_within_ms=[o["sync_ms_spread"] for o in offs],
               off_spread_between_ms=abs(offs[0]["sync_ms_median"] - offs[1]["sync_ms_median"]))
ctx.close()
finish(out)
