"""Cost record of cwslg_subtract_ft4 on the workload of scripts/ft4_decode_reports_cost.py at 1024 channels (FT4 channels on one
48 kHz receiver whose passbands carry synthetic FT4 transmissions plus --codewords transmissions that carry codewords of the test code; soft bits,
decode, OSD order 1).
  first call   the wall time of the context's FIRST cwslg_subtract_ft4, which loads the code object and allocates the residual block, on its own;
  per measured boundary, on the same epoch: ONE cwslg_subtract_ft4 beside ONE cwslg_fetch_ft4_decode_reports (decodes compared byte for byte), the
               same call with max = 0 (harvest and apply alone: the fit's share is the difference -- wall times, NOT HIP events: the library
               has no event pair around the module's launches), and stats.sync_ms of the boundary itself, which the call is no part of.
Median over the measured boundaries after a warm-up.

Per kernel: the script run once under a kernel trace (rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o sub -- python scripts/ft4_subtract_cost.py
--boundaries 3 --warmup 1 --out <elsewhere>); --finish reads <dir>/sub_kernel_stats.csv.  The boundary path: scripts/ft4_decode_reports_cost.py --sync-only runs of
the parent commit's checkout (--tree) and of this tree, alternating, and bench.py runs of both; --finish records them and reads them as DESIGN 4.14
reads its A/Bs: every run of this tree inside the parent's smallest-to-largest range widened by their difference.

    python scripts/ft4_subtract_cost.py [--channels 1024] [--boundaries 7] [--codewords 12] [--out profiles/ft4_subtract_cost.json]
    python scripts/ft4_subtract_cost.py --finish <this run's file> [--kernel-stats <csv>] [--parent-json <p1> ..] [--tree-sync-json <t1> ..] [--bench-json <file>]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--channels", type=int, default=1024)
ap.add_argument("--boundaries", type=int, default=7, help="measured boundaries (after --warmup)")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--max-cand", type=int, default=100)
ap.add_argument("--codewords", type=int, default=12)
ap.add_argument("--out", default=None)
ap.add_argument("--finish", default=None, help="no measurement: read this run's own result from the given file and add the other files")
ap.add_argument("--kernel-stats", default=None, help="kernel_stats.csv of a kernel-trace run of this script")
ap.add_argument("--parent-json", nargs="*", default=[], help="ft4_decode_reports_cost.py --sync-only runs of the parent commit's tree")
ap.add_argument("--tree-sync-json", nargs="*", default=[], help="the same of this tree, taken between the parent's runs")
ap.add_argument("--bench-json", default=None, help="{'parent': [bench.py result lines], 'tree': [...]}, runs alternating, parent first")
args = ap.parse_args()
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tests"))
sys.path.insert(0, HERE)


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
    for j in range(args.codewords):                                       # each lies in the passband of about sixty of 1024 channels
        cw = ldpc_cases.encode(seed, ldpc_cases.chain_message(900 + j))
        iq = iq + D.iq_of_tones(N, -20000.0 + 3300.0 * j + 137.5, 0.0, 0.4 + 0.05 * j, 3000.0, D.tones_of(cw))
    iq = iq.astype(np.complex64)

    ctx = P.Context(0)
    ctx.enable_sync(True, 1.5, args.max_cand, 200, 3000)
    ctx.enable_ft4_softbits(True)
    ctx.set_timing(True)
    ctx.set_ldpc_code(ldpc_cases.make_code(seed)["nm"])
    ctx.enable_ft4_decode(True, 30, 8, 20)
    ctx.enable_ft4_osd(True, 1, 8, 20)
    rx = ctx.receiver_open(FS, BLK, 0)
    chans = [ctx.channel_open(rx, int(f), "FT4") for f in np.linspace(-FS // 2 + 100, FS // 2 - 6600, args.channels).astype(int)]
    epoch = [10]
    ctx.slot_boundary("FT4", epoch[0])
    first = []

    def boundary():
        ctx.reset_stats()
        for k in range(0, N, 64 * BLK):
            ctx.push_iq(rx, iq[k:k + 64 * BLK])
        epoch[0] += 7
        ctx.slot_boundary("FT4", epoch[0])
        ctx.synchronize()
        s = ctx.stats()
        t0 = time.perf_counter()
        dec, sub, E, n_total, n_ch = ctx.subtract_ft4(0, 1 << 16)
        t1 = time.perf_counter()
        if not first:
            first.append(1e3 * (t1 - t0))
        rep = ctx.fetch_ft4_decode_reports(E, 1 << 16)
        t2 = time.perf_counter()
        ctx.subtract_ft4(E, 0)
        t3 = time.perf_counter()
        again = ctx.subtract_ft4(E, 1 << 16)
        t4 = time.perf_counter()
        assert n_ch == len(chans) and rep[0].tobytes() == dec.tobytes() == again[0].tobytes() and again[1].tobytes() == sub.tobytes()
        assert ctx.stats()["sync_launches"] == s["sync_launches"]
        return dict(sync_ms=s["sync_ms"], subtract_call_ms=1e3 * (t1 - t0), reports_call_ms=1e3 * (t2 - t1), subtract_max0_call_ms=1e3 * (t3 - t2),
                    subtract_second_call_ms=1e3 * (t4 - t3), n_total=int(n_total),
                    removed_over_before_median=float(np.median(sub["p_removed"] / np.maximum(sub["p_before"], 1e-30))) if len(sub) else None)

    rows = [boundary() for _ in range(args.warmup + args.boundaries)][args.warmup:]

    def summary(key):
        v = sorted(r[key] for r in rows)
        return dict(median=float(np.median(v)), min=float(v[0]), max=float(v[-1]), all=[round(float(r[key]), 4) for r in rows])

    out = dict(channels=args.channels, fs=FS, max_cand=args.max_cand, boundaries=args.boundaries, warmup=args.warmup, codewords=args.codewords,
               first_call_ms_with_module_load=first[0], subtract_call_ms=summary("subtract_call_ms"), subtract_second_call_ms=summary("subtract_second_call_ms"),
               reports_call_ms=summary("reports_call_ms"), subtract_max0_call_ms=summary("subtract_max0_call_ms"), sync_ms=summary("sync_ms"),
               n_total=sorted(set(r["n_total"] for r in rows)), removed_over_before_median=rows[-1]["removed_over_before_median"],
               residual_block_bytes=args.channels * 72576 * 4, fit_record_bytes_per_decode=26896,
               fit_kernel_resources=dict(vgpr=169, sgpr=96, lds_bytes=73104, scratch_bytes=0, workgroups_per_cu_by_lds=2, waves_per_simd=2),
               not_measured=["per-kernel times from HIP events (the fit's share is subtract_call_ms - subtract_max0_call_ms, wall time)",
                             "sync_ms of the parent commit's library on the same box (the boundary path's code is unchanged)",
                             "bench.py of the parent commit's tree on the same box"])
    ctx.close()
    return out


def _widened(values):
    lo, hi = min(values), max(values)
    return lo - (hi - lo), hi + (hi - lo)


def finish(out):
    if args.kernel_stats:
        import csv
        rows = {r["Name"]: r for r in csv.DictReader(open(args.kernel_stats))}
        out["kernel_trace"] = {k: dict(calls=int(v["Calls"]), avg_ms=float(v["AverageNs"]) * 1e-6, min_ms=float(v["MinNs"]) * 1e-6, max_ms=float(v["MaxNs"]) * 1e-6)
                               for k, v in rows.items() if k.startswith("ft4_sub_") or "decode_harvest_kernel" in k}
    if args.parent_json:
        par = [json.load(open(f))["sync_ms"] for f in args.parent_json]
        mine = [json.load(open(f))["sync_ms"] for f in args.tree_sync_json]
        lo, hi = _widened([q["median"] for q in par])
        out["boundary_path_ab"] = dict(workload="scripts/ft4_decode_reports_cost.py --sync-only (256 FT4 channels), child processes alternating, parent first",
                                       parent_sync_ms_medians=[round(q["median"], 4) for q in par], tree_sync_ms_medians=[round(q["median"], 4) for q in mine],
                                       bound=[round(lo, 4), round(hi, 4)], tree_runs_inside=bool(all(lo <= q["median"] <= hi for q in mine)))
    if args.bench_json:                                                   # the "value" of every result line (channel Msamples/s)
        b = json.load(open(args.bench_json))
        par, mine = [r["value"] for r in b["parent"]], [r["value"] for r in b["tree"]]
        lo, hi = _widened(par)
        out["bench_ab"] = dict(command="bench.py --gpus 1 --steps 5 --warmup 2, child processes alternating, parent first", metric=b["parent"][0].get("metric"),
                               unit=b["parent"][0].get("unit"), parent=par, tree=mine, bound=[lo, hi], tree_runs_inside=bool(all(lo <= v <= hi for v in mine)))
    drop = lambda m: (args.kernel_stats and m.startswith("per-kernel")) or (args.parent_json and m.startswith("sync_ms")) or (args.bench_json and m.startswith("bench.py"))
    out["not_measured"] = [m for m in out.get("not_measured", []) if not drop(m)]
    return out


out = finish(json.load(open(args.finish)) if args.finish else measure())
print(json.dumps(out))
path = args.out or os.path.join(HERE, "profiles", "ft4_subtract_cost.json")
with open(path, "w") as fh:            # one key per line
    fh.write("{\n" + ",\n".join(" %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in out.items()) + "\n}\n")
