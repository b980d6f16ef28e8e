"""Cost record of cwslg_fetch_ft4_decode_reports on the workload of scripts/ft4_decode_cost.py (256 FT4 channels on one 48 kHz receiver
whose passbands carry synthetic FT4 transmissions with random tones) plus --codewords transmissions that carry codewords of the test code, so that
the answer is not empty; soft bits, decode and OSD order 1 on.  Per measured boundary, in one process:
  (a) the wall time of ONE cwslg_fetch_ft4_decode_reports call beside ONE cwslg_fetch_decodes(FT4) call on the same epoch (each also repeated
      once); the decodes of the two are compared byte for byte, and at the first measured boundary every report is compared with
      tests/ft4_decode_reports_ref.py on the frame spectrum and sync records of its channel;
  (b) stats.sync_ms of the boundary itself, which the call is no part of (when this was recorded the soft-bit kernel hosted the report as a mode): to be set against the
      parent commit's library (--sync-only runs of a checkout of it, in processes of their own, alternating with --sync-only runs of this tree).
Median over the measured boundaries after a warm-up.

    python scripts/ft4_decode_reports_cost.py [--channels 256] [--boundaries 7] [--codewords 12] [--out profiles/ft4_decode_reports_cost.json]
    python scripts/ft4_decode_reports_cost.py --tree <other checkout> --sync-only --out <file>      # e.g. the parent commit's library
    python scripts/ft4_decode_reports_cost.py --finish <this run's file> --parent-json <p1> <p2> --tree-sync-json <t1> <t2> [--bench-json <file>]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--channels", type=int, default=256)
ap.add_argument("--boundaries", type=int, default=7, help="measured boundaries (after --warmup)")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--max-cand", type=int, default=100)
ap.add_argument("--max-iter", type=int, default=30)
ap.add_argument("--min-nsync", type=int, default=8)
ap.add_argument("--min-nqual", type=int, default=20)
ap.add_argument("--order", type=int, default=1)
ap.add_argument("--codewords", type=int, default=12, help="strong transmissions that carry codewords of the test code, so that the answer is not empty")
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose package and library are measured")
ap.add_argument("--sync-only", action="store_true", help="only (b): a tree that does not have the call")
ap.add_argument("--parent-json", nargs="*", default=[], help="results of --sync-only runs of the parent commit on the same box, recorded beside this run")
ap.add_argument("--tree-sync-json", nargs="*", default=[], help="results of --sync-only runs of THIS tree, taken between the parent's runs")
ap.add_argument("--bench-json", default=None, help="a file of bench.py result lines of both trees ({'tree': ..., 'parent': ...}), recorded beside this run")
ap.add_argument("--finish", default=None, help="no measurement: read this run's own result from the given file and add the other files")
ap.add_argument("--out", default=None)
args = ap.parse_args()
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tests"))
sys.path.insert(0, os.path.abspath(args.tree))


def measure():
    import cwsl_digi_amd as P                      # noqa: E402
    import ft4_decode_cases as D                   # noqa: E402
    import ldpc_cases                              # noqa: E402
    from ft4_softbits_ref import ft4_iq_with_tones  # noqa: E402

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
    checked = [0]

    def boundary(measured):
        ctx.reset_stats()
        for k in range(0, N, 64 * BLK):
            ctx.push_iq(rx, iq[k:k + 64 * BLK])
        epoch[0] += 7
        ctx.slot_boundary("FT4", epoch[0])
        ctx.synchronize()
        s = ctx.stats()
        row = dict(sync_ms=s["sync_ms"], sync_launches=int(s["sync_launches"]))
        if not args.sync_only:
            t0 = time.perf_counter()
            dec, rep, E, n_total, n_ch = ctx.fetch_ft4_decode_reports(0, 1 << 16)
            t1 = time.perf_counter()
            plain = ctx.fetch_decodes("FT4", E, 1 << 16)
            t2 = time.perf_counter()
            again = ctx.fetch_ft4_decode_reports(E, 1 << 16)
            t3 = time.perf_counter()
            plain2 = ctx.fetch_decodes("FT4", E, 1 << 16)
            t4 = time.perf_counter()
            assert n_ch == len(chans) and plain[1:] == (E, n_total, n_ch) and plain[0].tobytes() == dec.tobytes() == plain2[0].tobytes()
            assert again[0].tobytes() == dec.tobytes() and again[1].tobytes() == rep.tobytes() and ctx.stats()["sync_launches"] == s["sync_launches"]
            if measured and not checked[0]:                               # every report against the restatement, once
                import ft4_decode_reports_ref as R4
                import report_kernel_cases as K
                from oracle import oracle as orc
                ids = sorted({int(c) for c in dec["ch_id"]})
                want = R4.reports(orc, K.encoder(seed), {c: ctx.sync_debug(c, "ft4_cx") for c in ids}, {c: ctx.fetch_ft4_sync(c, 1800) for c in ids}, dec)
                assert want.tobytes() == rep.tobytes()
                checked[0] = len(dec)
            row.update(reports_call_ms=1e3 * (t1 - t0), decodes_call_ms=1e3 * (t2 - t1), reports_second_call_ms=1e3 * (t3 - t2), decodes_second_call_ms=1e3 * (t4 - t3),
                       n_total=int(n_total), n_clamped=int((rep["snr_db"] == -21).sum()), n_symerr_0=int((rep["nsymerr"] == 0).sum()),
                       snr_db_median=float(np.median(rep["snr_db"])) if len(rep) else None)
        return row

    for _ in range(args.warmup):
        boundary(False)
    rows = [boundary(True) for _ in range(args.boundaries)]

    def summary(key):
        v = sorted(r[key] for r in rows)
        return dict(median=float(np.median(v)), min=float(v[0]), max=float(v[-1]), all=[round(float(r[key]), 4) for r in rows])

    out = dict(channels=args.channels, fs=FS, max_cand=args.max_cand, boundaries=args.boundaries, warmup=args.warmup, osd_order=args.order, codewords=args.codewords,
               max_iter=args.max_iter, min_nsync=args.min_nsync, min_nqual=args.min_nqual, tree=os.path.basename(os.path.abspath(args.tree)),
               sync_ms=summary("sync_ms"), sync_launches_per_boundary=sorted(set(r["sync_launches"] for r in rows)))
    if not args.sync_only:
        out.update(reports_call_ms=summary("reports_call_ms"), decodes_call_ms=summary("decodes_call_ms"), reports_second_call_ms=summary("reports_second_call_ms"),
                   decodes_second_call_ms=summary("decodes_second_call_ms"), n_total=sorted(set(r["n_total"] for r in rows)),
                   n_clamped=sorted(set(r["n_clamped"] for r in rows)), n_symerr_0=sorted(set(r["n_symerr_0"] for r in rows)),
                   snr_db_median=rows[-1]["snr_db_median"], bytes_down_reports=[16 + 56 * r["n_total"] for r in rows][-1],
                   bytes_down_decodes=[16 + 40 * r["n_total"] for r in rows][-1], reports_checked_against_restatement=checked[0], decodes_equal=True)
    ctx.close()
    return out


out = json.load(open(args.finish)) if args.finish else measure()
parents = [json.load(open(p)) for p in args.parent_json]
trees = [json.load(open(p)) for p in args.tree_sync_json]
if args.bench_json:
    out["bench"] = json.load(open(args.bench_json))
if parents:
    # (b): this tree WITHOUT the call (--tree-sync-json; failing that, this run's own boundaries) against the parent's runs around it
    mine = trees or [out]
    lo = min(p["sync_ms"]["min"] for p in parents)
    hi = max(p["sync_ms"]["max"] for p in parents)
    tlo = min(t["sync_ms"]["min"] for t in mine)
    thi = max(t["sync_ms"]["max"] for t in mine)
    out.update(parent=[dict(tree=p["tree"], **p["sync_ms"]) for p in parents], parent_sync_ms_range=[lo, hi],
               tree_without_call=[dict(tree=t["tree"], **t["sync_ms"]) for t in trees], tree_sync_ms_range=[tlo, thi],
               tree_medians_inside_parent_range=bool(all(lo <= t["sync_ms"]["median"] <= hi for t in mine)),
               parent_medians_inside_tree_range=bool(all(tlo <= p["sync_ms"]["median"] <= thi for p in parents)))
print(json.dumps(out))
path = args.out or os.path.join(HERE, "profiles", "ft4_decode_reports_cost.json")
os.makedirs(os.path.dirname(path), exist_ok=True)
with open(path, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
