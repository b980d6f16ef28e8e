"""Test helper: the numpy restatement of FT4 a-priori decoding (include/cwsl_gpu.h, "FT4 a-priori decoding"), built on tests/ap_ref.py: the
setter's validation, the PER-RECORD gate over the three-set decode and OSD records, ap_ref.decode per metric set, the set-major choice and what
cwslg_fetch_ft4_ap hands out (tests/decodes_ref.py on the a-priori records, then by_osd = 2, set = s | p << 2, dmin).  PARITY UNPINNED like the
rest of the chain: this is the repository's own statement; the GPU (csrc/ap_kernels.hpp's FT4 addressing) is compared with it byte for byte.

Nothing per set is restated: rules 1 to 6 and the record rules are ap_ref.decode's."""
import numpy as np

import ap_ref as AP
import decodes_ref as DR
import ft4_decode_cases as D

F32 = np.float32
AP4_DTYPE = np.dtype([("set", AP.AP_MSG_DTYPE, 3)])
assert AP4_DTYPE.itemsize == 72


def validate(patterns, n_pat=None, max_iter=30, min_nsync=8, min_nqual=20):
    """What cwslg_set_ft4_ap answers: 0, or the reason -- 4 max_iter outside 1..200, min_nsync outside 0..17 or min_nqual outside 0..33 (checked
    first: cwslg_enable_ft4_decode's ranges), else ap_ref.validate's 1..3."""
    if not (1 <= max_iter <= 200) or not (0 <= min_nsync <= 17) or not (0 <= min_nqual <= 33):
        return 4
    return AP.validate(patterns, n_pat)


def taken(msg, osd, nsync, nqual, min_nsync, min_nqual):
    """bool[n]: the record is taken -- no set with BP crc_ok; the OSD records not used (osd None) or no set with OSD crc_ok; nsync and nqual pass."""
    t = ~(msg["set"]["crc_ok"] != 0).any(axis=1) & (np.asarray(nsync) >= min_nsync) & (np.asarray(nqual) >= min_nqual)
    if osd is not None:
        t &= ~(osd["set"]["crc_ok"] != 0).any(axis=1)
    return t


def gate(msg, osd, nsync, nqual, min_nsync, min_nqual):
    """bool[n, 3]: set s of record q is attempted (rule 1, the finite metrics, is ap_ref.decode's to add) iff the record is taken and the decode
    attempted that set."""
    return (msg["set"]["iters"] >= 0) & taken(msg, osd, nsync, nqual, min_nsync, min_nqual)[:, None]


def decode(code, soft, msg, osd, patterns, max_iter, min_nsync, min_nqual, loop=AP.bp):
    """soft: dict(llr [n, 3, 174], nsync [n], nqual [n], ...); msg: cwslg_ft4_msg records [n]; osd: cwslg_ft4_osd records [n] or None (not used)
    -> AP4_DTYPE[n]: set s is ap_ref.decode of llr[:, s] under gate()."""
    n = len(msg)
    out = np.zeros(n, AP4_DTYPE)
    if n == 0:
        return out
    att = gate(msg, osd, soft["nsync"], soft["nqual"], min_nsync, min_nqual)
    llr = np.asarray(soft["llr"], F32).reshape(n, 3, 174)
    for s in range(3):
        out["set"][:, s] = AP.decode(code, llr[:, s], patterns, max_iter, att[:, s], loop=loop)
    return out


def best_set(ap):
    """The smallest s whose a-priori record has crc_ok, -1 if none: int array [n].  Set-major: the pattern index plays no part."""
    ok = ap["set"]["msg"]["crc_ok"] != 0
    return np.where(ok.any(axis=1), ok.argmax(axis=1), -1)


def set_byte(s, p):
    """cwslg_decode.set of an FT4 a-priori record."""
    return int(s) | int(p) << 2


def split(set_byte_):
    return int(set_byte_) & 3, int(set_byte_) >> 2


def ap_decodes(channels, max_out=None):
    """What cwslg_fetch_ft4_ap hands out.  channels: [(ch_id, where, ap records AP4_DTYPE)] of the channels that take part (where: decodes_ref's
    where_ft4 of the sync records in compacted order): decodes_ref's FT4 rules on the a-priori records in the decode records' place and no OSD
    records, then by_osd = 2, set = s | p << 2 and dmin = that a-priori record's."""
    as_msg = []
    for c, w, a in channels:
        m = np.zeros(len(a), D.MSG4_DTYPE)
        m["set"] = a["set"]["msg"]
        as_msg.append((c, w, m, None))
    rec, n_total = DR.decodes("FT4", as_msg, max_out)
    by_ch = {c: a for c, w, a in channels}
    for r in rec:
        s = int(r["set"])
        a = by_ch[int(r["ch_id"])][int(r["entry"])]["set"][s]
        r["by_osd"], r["set"], r["dmin"] = 2, set_byte(s, a["msg"]["pad_"]), a["dmin"]
    return rec, n_total
