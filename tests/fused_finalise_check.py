"""Test helper: the slot finalise (prepareAudio + int16, Instance.cpp:294-338, 238-241) on the CPU, twice, and a per-slot checker of what a boundary
left on the GPU.

Since round 6 the finalise of FT8 channels with the sync stage on runs inside symbol_spectra_v2_kernel: every workgroup converts the samples its own
windows cover, stores them as int16 and reads them back as windows two transforms later; neighbouring workgroups both store the samples they share, to
the same bits.  A window that was read back stale therefore leaves the int16 FRAME in memory right and the SPECTRA PLANE (and the list made from it)
wrong -- so check_slot recomputes the plane and the list from the final int16 frame, and the frame itself from the GPU's own float frame.  None of
this depends on the arithmetic mode of the demodulator: every comparison is on bits, in exact and in fast mode alike.

The CPU work (2 + 60 + 68 ms per FT8 frame on one thread; the ctypes calls release the GIL) goes to a small thread pool with a bounded queue; every
GPU call stays on the calling thread.
"""
import os
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np

FT8_NSTEP, FT8_NHSYM, FT8_NSPS = 480, 372, 1920          # a symbol step, steps per frame, samples per window (sync_kernels.hpp)
FT8_COVER = FT8_NSTEP * (FT8_NHSYM - 1) + FT8_NSPS       # 180 000: the samples the windows cover; the frame beyond is its tail


def spectra_jper(n_ft8):
    """Symbol steps per workgroup of symbol_spectra_v2_kernel for a boundary with n_ft8 FT8 channels (spectra_jper, sync_kernels.hpp): the longest of
    62 / 31 that still gives 3072 workgroups, else 12."""
    for jper in (62, 31):
        if n_ft8 * ((FT8_NHSYM + jper - 1) // jper) >= 3072:
            return jper
    return 12


def _scale(mode):
    return 0.20 if mode == "WSPR" else 0.90              # Instance.cpp:320: an exact compare with "WSPR"; FST4W-120 takes the FT factor


def _valid(a_f32, n_valid):
    a = np.asarray(a_f32, np.float32)
    x = np.zeros(len(a), np.float32)
    x[:n_valid] = a[:n_valid]
    return x


def cpu_finalise(a_f32, n_valid, mode):
    """(int16 frame, factor) of the float frame a[:n_valid] by the oracle's prepare_audio + to_int16; everything at and beyond n_valid counts as zero,
    whatever the fetched buffer holds there."""
    from oracle import oracle as O
    scaled, factor, _ = O.prepare_audio(_valid(a_f32, n_valid), mode)
    return O.to_int16(scaled), np.float32(factor)


def numpy_finalise(a_f32, n_valid, mode):
    """The same in plain numpy float32: peak = max|x|; factor = 32767 / (peak + 1), then * scale (two roundings); (x * factor + 0.5f) truncated
    toward zero and narrowed to int16."""
    x = _valid(a_f32, n_valid)
    peak = np.float32(np.abs(x).max()) if len(x) else np.float32(0)
    factor = np.float32(32767.0) / (peak + np.float32(1.0))
    factor = np.float32(factor * np.float32(_scale(mode)))
    y = (x * factor).astype(np.float32) + np.float32(0.5)
    return np.trunc(y).astype(np.int32).astype(np.int16), factor


def _u32(x):
    return np.float32(x).view(np.uint32)


def cand_bits(cands):
    """A candidate list with every float as its uint32 view."""
    return [tuple(int(_u32(v)) if isinstance(v, float) else int(v) for v in c) for c in cands]


def _where(i, jper, what):
    j = min(int(i) // FT8_NSTEP, FT8_NHSYM - 1)
    wg = f", workgroup {j // jper} of jper {jper}" if jper else ""
    return f"{what} {int(i)} (symbol step {j}{wg})"


def check_slot(ctx, oracle, ch, mode, sync_params=None, tag=None):
    """Fetch what the last boundary left for channel `ch` (GPU calls, on the calling thread) and return a job for a worker: job() does the CPU work
    and raises AssertionError on the first mismatch; job.fetched is a dict with the frame (i16, t_start, n_valid, factor), the float frame f32
    and -- for FT8 with the sync stage on -- plane and cands.  sync_params: None (no FT8 sync stage for this channel) or dict(lo, hi, syncmin, maxcand[, order,
    jper]); jper only labels failures."""
    name = f"slot {tag if tag is not None else ch} ({mode}, {getattr(ctx, 'mode', '?')} mode)"
    g = ctx.fetch_frame(ch)
    assert g is not None, f"{name}: no frame"
    a, nv = ctx.fetch_audio_f32(ch)
    got = dict(g, f32=a)
    ft8 = mode == "FT8" and sync_params is not None
    if ft8:
        got["plane"] = ctx.sync_debug(ch, "spectra")
        got["cands"] = ctx.fetch_candidates(ch, max(600, sync_params["maxcand"]))
    jper = (sync_params or {}).get("jper", 0)

    def job():
        i16, n_valid = got["i16"], int(got["n_valid"])
        assert n_valid == int(nv), f"{name}: n_valid {n_valid} from fetch_frame, {nv} from fetch_audio_f32"
        assert len(i16) == len(a) and 0 <= n_valid <= len(i16), f"{name}: frame lengths {len(i16)} / {len(a)}, n_valid {n_valid}"
        ref, factor = cpu_finalise(a, n_valid, mode)
        assert _u32(got["factor"]) == _u32(factor), f"{name}: factor {got['factor']!r} ({_u32(got['factor']):#x}), CPU finalise {factor!r} ({_u32(factor):#x})"
        bad = np.nonzero(i16 != ref)[0]
        assert bad.size == 0, (f"{name}: {bad.size} int16 samples differ from the finalise of the GPU's own float frame, first at "
                               f"{_where(bad[0], jper, 'sample')}: {i16[bad[0]]} for {ref[bad[0]]}; n_valid {n_valid}")
        tail = np.nonzero(i16[n_valid:])[0]
        assert tail.size == 0, f"{name}: {tail.size} non-zero samples at and beyond n_valid {n_valid}, first at {_where(n_valid + tail[0], jper, 'sample')}"
        if not ft8:
            return
        p = sync_params
        plane = got["plane"]
        nbins = plane.shape[1]
        assert plane.shape[0] == FT8_NHSYM, f"{name}: plane of {plane.shape}"
        want = oracle.ft8_spectra(i16, nbins)
        badp = np.nonzero(plane.view(np.uint32).ravel() != want.view(np.uint32).ravel())[0]
        if badp.size:
            j, k = divmod(int(badp[0]), nbins)
            wg = f", workgroup {j // jper} of jper {jper}" if jper else ""
            raise AssertionError(f"{name}: {badp.size} values of the spectra plane differ from the restatement on the final int16 frame, first at flat "
                                 f"index {int(badp[0])} (symbol step {j}, bin {k}{wg}): {plane[j, k]!r} for {want[j, k]!r}; "
                                 f"{len(np.unique(badp // nbins))} steps affected; n_valid {n_valid}")
        lst = oracle.ft8_sync(i16, p["lo"], p["hi"], p["syncmin"], p["maxcand"], order=p.get("order", "sync"))
        assert cand_bits(got["cands"]) == cand_bits(lst), f"{name}: candidate list differs from the restatement's on the final int16 frame ({len(got['cands'])} / {len(lst)} entries)"

    job.fetched = got
    return job


class SlotJobs:
    """A pool for check_slot's jobs: min(16, CPUs this process may use) workers, at most `depth` slots in flight -- submit() waits for the oldest
    beyond that -- so a run over thousands of slots never holds more than a few dozen frames and planes.  A failed job raises from submit() or drain()."""

    def __init__(self, depth=48):
        self.pool = ThreadPoolExecutor(max_workers=min(16, len(os.sched_getaffinity(0))))
        self.depth = depth
        self.pending = deque()
        self.done = 0

    def submit(self, job):
        self.pending.append(self.pool.submit(job))
        while len(self.pending) >= self.depth:
            self.pending.popleft().result()
            self.done += 1

    def drain(self):
        try:
            while self.pending:
                self.pending.popleft().result()
                self.done += 1
        finally:
            for f in self.pending:
                f.cancel()
            self.pending.clear()

    def close(self):
        for f in self.pending:
            f.cancel()
        self.pool.shutdown(wait=True)

    def __enter__(self):
        return self

    def __exit__(self, et, ev, tb):
        try:
            if et is None:
                self.drain()
        finally:
            self.close()
        return False
