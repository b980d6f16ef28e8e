"""Test helper: the numpy restatement of cwslg_fetch_decodes (include/cwsl_gpu.h, "The decodes of a slot") -- what the call hands out for a
slot-clock group, computed from the per-channel records the other fetches return.  Plain loops over plain records: nothing here is shaped like
the kernel (no compaction, no prefix, no LDS list).

The contract, restated:
  1. group is the FT8 or the FT4 slot-clock group; a null ctx, start_epoch, n or n_total, or dst null with max > 0, is CWSLG_ERR_ARG.
  2. A channel takes part only if it is open, belongs to the group, has that chain's sync stage (a JS8 channel does not) and its decode records
     may be handed out under an epoch E_ch != 0.  E = *start_epoch, or the largest E_ch if that is 0; the channels with E_ch == E take part; none:
     CWSLG_ERR_NO_FRAME with all counts 0.  (The CALLER of this module decides that: `channels` below holds the channels that take part.)
  3. A channel's OSD records are used only if they are also of epoch E (here: osd is not None).
  4. The entries are all min(count, max_cand) entries of the list (FT4: the sync records in compacted order).  FT8: the word is the decode
     record's if msg.crc_ok; otherwise, if OSD is used and osd.crc_ok, the OSD record's.  FT4: the smallest set with BP crc_ok; failing that,
     the smallest set with OSD crc_ok.  An entry without a word contributes nothing; neither does a word whose 91 bits are all zero.
  5. Per channel, entries with equal bits are one decode; the entry reported is the smallest by (by_osd, nharderr, entry); ndup counts all
     entries that carried the word (saturating at 65535).
  6. Output order: ascending ch_id, then ascending entry.  n_total counts every decode; n = min(n_total, max); the first n are written.
  7. The call changes nothing (the GPU tests check that around it)."""
import numpy as np

DECODE_DTYPE = np.dtype([("ch_id", np.int32), ("entry", np.int16), ("by_osd", np.uint8), ("set", np.uint8), ("bits", np.uint8, 12), ("freq_hz", np.float32),
                         ("dt_s", np.float32), ("sync", np.float32), ("dmin", np.float32), ("nharderr", np.int16), ("ndup", np.uint16)])
assert DECODE_DTYPE.itemsize == 40


def all_zero_word(bits):
    """The 91 bits of a word (12 bytes, MSB first; the last 5 bits are padding) are all zero."""
    b = bytes(bytearray(bits))
    return not any(b[:11]) and (b[11] & 0xE0) == 0


def _word_ft8(msg, osd):
    """-> None, or (by_osd, set, bits, nharderr, dmin) of one FT8 entry."""
    if msg["crc_ok"]:
        return 0, 0, bytes(bytearray(msg["bits"])), int(msg["nharderr"]), np.float32(0.0)
    if osd is not None and osd["crc_ok"]:
        return 1, 0, bytes(bytearray(osd["bits"])), int(osd["nharderr"]), np.float32(osd["dmin"])
    return None


def _word_ft4(msg, osd):
    """-> None, or (by_osd, set, bits, nharderr, dmin) of one FT4 entry: the rule of ft4_best_word."""
    for s in range(3):
        if msg["set"][s]["crc_ok"]:
            return 0, s, bytes(bytearray(msg["set"][s]["bits"])), int(msg["set"][s]["nharderr"]), np.float32(0.0)
    if osd is not None:
        for s in range(3):
            if osd["set"][s]["crc_ok"]:
                return 1, s, bytes(bytearray(osd["set"][s]["bits"])), int(osd["set"][s]["nharderr"]), np.float32(osd["set"][s]["dmin"])
    return None


def channel_decodes(mode, ch_id, where, msg, osd):
    """The decodes of one channel, in ascending entry.  where: per entry (freq_hz, dt_s, sync) -- FT8: the candidate's freq_hz, dt_s, sync; FT4:
    the sync record's f1_hz, dt_s, sync; msg / osd: the decode / OSD records of the same entries (osd None: OSD is not used).  Entry q is index q
    of `where`, `msg` and `osd` alike."""
    assert len(msg) == len(where) and (osd is None or len(osd) == len(msg)), (len(where), len(msg), None if osd is None else len(osd))
    words = []
    for q in range(len(msg)):
        w = (_word_ft8 if mode == "FT8" else _word_ft4)(msg[q], None if osd is None else osd[q])
        if w is not None and not all_zero_word(w[2]):
            words.append((q,) + w)
    out = []
    for q, by_osd, s, bits, nharderr, dmin in words:
        same = [(o_by, o_nh, o_q) for o_q, o_by, _, o_bits, o_nh, _ in words if o_bits == bits]
        if min(same) != (by_osd, nharderr, q):
            continue
        rec = np.zeros((), DECODE_DTYPE)
        rec["ch_id"], rec["entry"], rec["by_osd"], rec["set"] = ch_id, q, by_osd, s
        rec["bits"] = np.frombuffer(bits, np.uint8)
        rec["freq_hz"], rec["dt_s"], rec["sync"] = (np.float32(v) for v in where[q])
        rec["dmin"], rec["nharderr"], rec["ndup"] = dmin, nharderr, min(len(same), 65535)
        out.append(rec)
    return out


def decodes(mode, channels, max_out=None):
    """channels: [(ch_id, where, msg, osd)] of the channels that take part, in any order.  -> (records, n_total): the first min(n_total, max_out)
    decodes (all of them for max_out None) as a DECODE_DTYPE array, ascending ch_id then entry."""
    out = []
    for ch_id, where, msg, osd in sorted(channels, key=lambda c: c[0]):
        out += channel_decodes(mode, ch_id, where, msg, osd)
    n_total = len(out)
    if max_out is not None:
        out = out[:max(int(max_out), 0)]
    return (np.array(out, DECODE_DTYPE) if out else np.zeros(0, DECODE_DTYPE)), n_total


def where_ft8(cands):
    """(freq_hz, dt_s, sync) per candidate tuple (freq_bin, time_step, sync, freq_hz, dt_s)."""
    return [(c[3], c[4], c[2]) for c in cands]


def where_ft4(recs):
    """(f1_hz, dt_s, sync) per sync record (dicts as fetch_ft4_sync returns them)."""
    return [(r["f1_hz"], r["dt_s"], r["sync"]) for r in recs]
