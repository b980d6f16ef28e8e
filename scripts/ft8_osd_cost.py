"""Cost record of the FT8 OSD launch (cwslg_enable_ft8_osd): stats.sync_ms per boundary with soft bits and the decode on in every leg and OSD off,
on at order 1, on at order 2 and off again -- same process, same box -- on the workload of scripts/ft8_decode_cost.py: 1024 or more FT8 channels
whose passbands carry synthetic transmissions (tests/ft8_signal.py) with random tones, not codewords, so nearly every attempted candidate fails
belief propagation and goes on to OSD: the bulk of any real list.  Median over the measured boundaries after a warm-up; the two "off" legs
bracket the "on" legs.  The code is one of the test codes (tests/ldpc_cases.py).

    python scripts/ft8_osd_cost.py [--channels 1024] [--boundaries 7] [--out profiles/ft8_osd_cost.json]
    python scripts/ft8_osd_cost.py --tree <other checkout> --off-only --out <file>    # e.g. the parent commit's library: soft bits and decode on, no OSD
    python scripts/ft8_osd_cost.py --finish <this run's file> --parent-json <before> <after>    # no measurement: add the parent's runs to a finished record
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
ap.add_argument("--max-iter", type=int, default=30)
ap.add_argument("--min-nsync", type=int, default=7)
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose package and library are measured")
ap.add_argument("--off-only", action="store_true", help="only the OSD-off leg (a tree that does not have the feature)")
ap.add_argument("--parent-json", nargs="*", default=[], help="results of --off-only runs of the parent commit on the same box, recorded beside this run")
ap.add_argument("--finish", default=None, help="no measurement: read this run's own result from the given file and add --parent-json (the parent's second run comes after it)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert args.channels >= 1024 and args.boundaries >= 5
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tests"))
sys.path.insert(0, os.path.abspath(args.tree))
def measure():
    import cwsl_digi_amd as P                      # noqa: E402
    import ldpc_cases                              # noqa: E402
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
    ctx.enable_ft8_softbits(True)
    ctx.set_timing(True)
    ctx.set_ldpc_code(ldpc_cases.make_code(ldpc_cases.SEEDS[0])["nm"])
    ctx.enable_ft8_decode(True, args.max_iter, args.min_nsync)
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
        return s["sync_ms"], s["sync_launches"]


    def leg(order):
        """order None: leave the context as it is (a tree without the feature); -1: OSD off; 0..2: on."""
        if order is not None:
            ctx.enable_ft8_osd(order >= 0, max(order, 0), args.min_nsync)
        for _ in range(args.warmup):
            boundary()
        rows = [boundary() for _ in range(args.boundaries)]
        ms = sorted(r[0] for r in rows)
        out = dict(sync_ms_median=float(np.median(ms)), sync_ms_min=ms[0], sync_ms_max=ms[-1], sync_ms=[round(r[0], 4) for r in rows],
                   sync_launches_per_boundary=sorted(set(int(r[1]) for r in rows)))
        if order is not None and order >= 0:                                # the records of the leg's last boundary
            total = attempted = crc_ok = 0
            hows = np.zeros(3, int)
            for ch in chans:
                rec = ctx.fetch_ft8_osd(ch, args.max_cand)
                assert rec is not None and len(rec) == len(ctx.fetch_candidates(ch, args.max_cand))
                att = rec["how"] != 0xff
                total += len(rec); attempted += int(att.sum()); crc_ok += int(rec["crc_ok"].sum())
                hows += np.bincount(rec["how"][att], minlength=3)[:3]
            out.update(candidates_total=total, attempted=attempted, attempted_share=attempted / max(total, 1), crc_ok=crc_ok, winners_by_flips=[int(h) for h in hows])
        return out


    out = dict(channels=args.channels, fs=FS, max_cand=args.max_cand, boundaries=args.boundaries, warmup=args.warmup,
               soft_bits_and_decode="on in every leg", max_iter=args.max_iter, min_nsync=args.min_nsync, tree=os.path.basename(os.path.abspath(args.tree)))
    if args.off_only:
        out["off"] = leg(None)
    else:
        out["off"] = leg(-1)
        out["order1"] = leg(1)
        out["order2"] = leg(2)
        out["off_again"] = leg(-1)
        offs = (out["off"], out["off_again"])
        base = 0.5 * (offs[0]["sync_ms_median"] + offs[1]["sync_ms_median"])
        for name in ("order1", "order2"):
            o = out[name]
            o["added_sync_ms"] = o["sync_ms_median"] - base
            o["added_us_per_attempted"] = 1e3 * o["added_sync_ms"] / max(o["attempted"], 1)
        out.update(off_spread_within_ms=[o["sync_ms_max"] - o["sync_ms_min"] for o in offs],
                   off_spread_between_ms=abs(offs[0]["sync_ms_median"] - offs[1]["sync_ms_median"]))
    ctx.close()
    return out


if args.finish:
    out = json.load(open(args.finish))
else:
    out = measure()
if not args.off_only:
    offs = (out["off"], out["off_again"])
    parents = [json.load(open(p)) for p in args.parent_json]
    if parents:
        lo = min(p["off"]["sync_ms_min"] for p in parents)
        hi = max(p["off"]["sync_ms_max"] for p in parents)
        out.update(parent=[dict(tree=p["tree"], **p["off"]) for p in parents], parent_sync_ms_medians=[p["off"]["sync_ms_median"] for p in parents],
                   parent_sync_ms_range=[lo, hi], off_inside_parent_range=bool(all(lo <= o["sync_ms_median"] <= hi for o in offs)))
print(json.dumps(out))
path = args.out or os.path.join(HERE, "profiles", "ft8_osd_cost.json")
os.makedirs(os.path.dirname(path), exist_ok=True)
with open(path, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
