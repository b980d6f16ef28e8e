"""Cost record of cwslg_fetch_ft4_ap on the workload of scripts/ft4_decode_reports_cost.py (256 FT4 channels on one 48 kHz receiver
whose passbands carry synthetic FT4 transmissions with random tones and twelve strong ones that carry codewords), soft bits, decode and OSD
order 1 on.  Per measured boundary, in one process: the wall time of ONE cwslg_fetch_decodes(FT4) call and of ONE cwslg_fetch_ft4_ap call under 1
and under 4 patterns on the same epoch (pattern 0: the first 29 bits of the first codeword's message; the others: random fields), each also
repeated once, the decodes each returns, how many records the a-priori gate takes and how many sets its launch attempts, and stats.sync_ms of the
boundary, which the calls are no part of.  Median over the measured boundaries after a warm-up.  What a boundary costs WITHOUT the call -- the
hosting kernel runs at every FT4 and FT8 boundary -- is parent against tree: scripts/ft4_decode_reports_cost.py --sync-only (FT4) and
scripts/fetch_decodes_cost.py --sync-only --codewords 12 (FT8) on a checkout of each, one process per run, alternating; --finish records those
runs and bench.py's lines here.

    python scripts/ft4_ap_cost.py [--channels 256] [--boundaries 7] [--out profiles/ft4_ap_cost.json]
    python scripts/ft4_ap_cost.py --finish <this run's file> --sync-json ft4:parent=<f> ft4:tree=<f> ft8:parent=<f> ... --bench-json parent=<f> tree=<f> ...
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--channels", type=int, default=256)
ap.add_argument("--boundaries", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--max-cand", type=int, default=100)
ap.add_argument("--max-iter", type=int, default=30)
ap.add_argument("--min-nsync", type=int, default=8)
ap.add_argument("--min-nqual", type=int, default=20)
ap.add_argument("--order", type=int, default=1)
ap.add_argument("--codewords", type=int, default=12)
ap.add_argument("--sync-json", nargs="*", default=[], help="mode:side=file triples (mode ft4 / ft8, side parent / tree): --sync-only results, in the order they were made")
ap.add_argument("--bench-json", nargs="*", default=[], help="side=file pairs: the JSON line of a bench.py run, in the order they were made")
ap.add_argument("--finish", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tests"))
sys.path.insert(0, HERE)


def measure():
    import cwsl_digi_amd as P
    import ap_ref
    import ft4_ap_ref
    import ft4_decode_cases as D
    import ldpc_cases
    from ft4_softbits_ref import ft4_iq_with_tones

    FS, BLK = 48000, 1024
    N = int(7.5 * FS) // BLK * BLK
    rng = np.random.default_rng(1)
    iq = (rng.normal(0.0, 30.0, N) + 1j * rng.normal(0.0, 30.0, N)).astype(np.complex64)
    for k, rf in enumerate(np.arange(-23500.0, 23500.0, 450.0)):          # a transmission every 450 Hz: six or seven in every 3 kHz passband
        iq = iq + ft4_iq_with_tones(FS, N, rf, 0.0, 0.05 + 0.17 * (k % 9), 1500.0 + 250.0 * (k % 5), 100 + k)[0]
    seed = ldpc_cases.SEEDS[0]
    for j in range(args.codewords):                                       # each lies in the passband of about fifteen of 256 channels
        cw = ldpc_cases.encode(seed, ldpc_cases.chain_message(900 + j))
        iq = iq + D.iq_of_tones(N, -20000.0 + 3300.0 * j + 137.5, 0.0, 0.4 + 0.05 * j, 3000.0, D.tones_of(cw))
    iq = iq.astype(np.complex64)
    prng = np.random.default_rng(7)
    fields = [ldpc_cases.chain_message(900)[:29]] + [prng.integers(0, 2, 29) for _ in range(3)]
    pats = ap_ref.make_patterns([(np.ones(29, np.uint8), f) for f in fields])

    ctx = P.Context(0)
    ctx.enable_sync(True, 1.5, args.max_cand, 200, 3000)
    ctx.enable_ft4_softbits(True)
    ctx.set_timing(True)
    ctx.set_ldpc_code(ldpc_cases.make_code(seed)["nm"])
    ctx.enable_ft4_decode(True, args.max_iter, args.min_nsync, args.min_nqual)
    ctx.enable_ft4_osd(True, args.order, args.min_nsync, args.min_nqual)
    rx = ctx.receiver_open(FS, BLK, 0)
    freqs = np.linspace(-FS // 2 + 100, FS // 2 - 6600, args.channels).astype(int)
    chans = [ctx.channel_open(rx, int(f), "FT4") for f in freqs]
    epoch = [10]
    ctx.slot_boundary("FT4", epoch[0])

    def timed(fn, *a):
        t0 = time.perf_counter()
        r = fn(*a)
        return r, 1e3 * (time.perf_counter() - t0)

    def boundary(last=False):
        ctx.reset_stats()
        for k in range(0, N, 64 * BLK):
            ctx.push_iq(rx, iq[k:k + 64 * BLK])
        epoch[0] += 7
        ctx.slot_boundary("FT4", epoch[0])
        ctx.synchronize()
        s = ctx.stats()
        row = dict(sync_ms=s["sync_ms"], sync_launches=int(s["sync_launches"]))
        dec, row["decodes_call_ms"] = timed(ctx.fetch_decodes, "FT4", 0, 1 << 16)
        row["decodes_n_total"] = int(dec[2])
        for n_pat in (1, 4):
            ctx.set_ft4_ap(pats[:n_pat], args.max_iter, args.min_nsync, args.min_nqual)
            got, row["ap%d_call_ms" % n_pat] = timed(ctx.fetch_ft4_ap, 0, 1 << 16)
            again, row["ap%d_second_call_ms" % n_pat] = timed(ctx.fetch_ft4_ap, got[1], 1 << 16)
            assert again[0].tobytes() == got[0].tobytes() and got[3] == len(chans) and (got[0]["by_osd"] == 2).all()
            row["ap%d_n_total" % n_pat] = int(got[2])
            row["ap%d_new_words" % n_pat] = int(len(P.api.merge_ap_decodes(dec[0], got[0])) - len(dec[0]))
        assert ctx.stats()["sync_launches"] == s["sync_launches"]
        if last:                                                    # how much work the a-priori launch had: the records and sets behind its gate
            records = taken = sets = 0
            for ch in chans:
                msg, osd, soft = ctx.fetch_ft4_decode(ch, 3 * args.max_cand), ctx.fetch_ft4_osd(ch, 3 * args.max_cand), ctx.fetch_ft4_softbits(ch, 3 * args.max_cand)
                records += len(msg)
                taken += int(ft4_ap_ref.taken(msg, osd, soft[2], soft[3], args.min_nsync, args.min_nqual).sum())
                sets += int((ft4_ap_ref.gate(msg, osd, soft[2], soft[3], args.min_nsync, args.min_nqual) & np.isfinite(soft[0]).all(axis=2)).sum())
            row.update(records=records, taken=taken, sets=sets)
        return row

    for _ in range(args.warmup):
        boundary()
    rows = [boundary(last=(k == args.boundaries - 1)) for k in range(args.boundaries)]

    def summary(key):
        v = sorted(r[key] for r in rows)
        return dict(median=float(np.median(v)), min=float(v[0]), max=float(v[-1]), all=[round(float(r[key]), 4) for r in rows])

    out = dict(channels=args.channels, fs=FS, max_cand=args.max_cand, boundaries=args.boundaries, warmup=args.warmup, osd_order=args.order,
               codewords=args.codewords, max_iter=args.max_iter, min_nsync=args.min_nsync, min_nqual=args.min_nqual, known_bits=29,
               sync_ms_with_the_calls_between_boundaries=summary("sync_ms"), sync_launches_per_boundary=sorted(set(r["sync_launches"] for r in rows)),
               records=rows[-1]["records"], records_taken_by_ap=rows[-1]["taken"], sets_attempted_by_ap=rows[-1]["sets"])
    for key in ("decodes_call_ms", "ap1_call_ms", "ap1_second_call_ms", "ap4_call_ms", "ap4_second_call_ms"):
        out[key] = summary(key)
    for key in ("decodes_n_total", "ap1_n_total", "ap1_new_words", "ap4_n_total", "ap4_new_words"):
        out[key] = sorted(set(r[key] for r in rows))
    ctx.close()
    return out


out = json.load(open(args.finish)) if args.finish else dict(cost=measure())
cost = out["cost"]
by_mode = {}
for item in args.sync_json:
    key, path = item.split("=", 1)
    mode, side = key.split(":")
    by_mode.setdefault(mode, []).append((side, json.load(open(path))["sync_ms"]))
for mode, runs in by_mode.items():
    par = [r for s, r in runs if s == "parent"]
    tre = [r for s, r in runs if s == "tree"]
    lo, hi = min(p["min"] for p in par), max(p["max"] for p in par)
    mlo, mhi = min(p["median"] for p in par), max(p["median"] for p in par)
    cost["sync_ms_without_the_call_" + mode] = dict(order=[s for s, _ in runs], parent=par, tree=tre, parent_range=[lo, hi], parent_median_range=[mlo, mhi],
                                                    tree_medians_inside_parent_range=bool(all(lo <= t["median"] <= hi for t in tre)),
                                                    tree_medians_inside_parent_median_range=bool(all(mlo <= t["median"] <= mhi for t in tre)))
if args.bench_json:
    runs = []
    for item in args.bench_json:
        side, path = item.split("=", 1)
        line = [l for l in open(path).read().splitlines() if l.startswith("{")][-1]
        runs.append(dict(side=side, ms_per_step=json.loads(line)["ms_per_step"]))
    cost["bench_py_gpus1_steps10_warmup3"] = runs
print(json.dumps(out))
path = args.out or os.path.join(HERE, "profiles", "ft4_ap_cost.json")
if os.path.isfile(path):                                           # the file's other sections (what AP is worth, the kernel's resources) stay
    out = dict(json.load(open(path)), cost=cost)
with open(path, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
