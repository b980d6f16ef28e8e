"""CPU: tests/decodes_ref.py, the restatement of cwslg_fetch_decodes, on hand-made records -- every rule of the contract once, with the answer
written out by hand."""
import os

import numpy as np

import decodes_ref as DR
import ft4_decode_cases as D4
import ft4_osd_cases as X4
import ldpc_ref as R
import osd_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(v):
    """A 12-byte word from a small integer: distinct integers give distinct words, 0 gives the all-zero word."""
    return np.frombuffer(int(v << 5).to_bytes(12, "big"), np.uint8)


def _msg(word=None, nharderr=0):
    """One cwslg_ft8_msg: word None = BP failed (bits are whatever BP left: here a word that must never be reported)."""
    r = np.zeros((), R.MSG_DTYPE)
    r["bits"], r["crc_ok"], r["nharderr"], r["iters"] = _bits(0x7777 if word is None else word), word is not None, nharderr, 3
    return r


def _osd(word=None, nharderr=0, dmin=0.0):
    r = np.zeros((), O.OSD_DTYPE)
    r["bits"], r["crc_ok"], r["nharderr"], r["dmin"] = _bits(0x5555 if word is None else word), word is not None, nharderr, dmin
    return r


def _where(n):
    return [(100.0 + q, 0.5 + 0.01 * q, 2.0 + q) for q in range(n)]


def _ft8(msgs, osds=None):
    return np.array(msgs, R.MSG_DTYPE), None if osds is None else np.array(osds, O.OSD_DTYPE)


def _rows(recs):
    return [(int(r["ch_id"]), int(r["entry"]), int(r["by_osd"]), int(r["set"]), int.from_bytes(bytes(r["bits"]), "big") >> 5, int(r["nharderr"]),
             int(r["ndup"])) for r in recs]


def test_layout_is_the_headers():
    src = open(os.path.join(ROOT, "include", "cwsl_gpu.h")).read()
    body = src[src.index("typedef struct {\n    int32_t  ch_id;"):src.index("} cwslg_decode;")]
    names = [ln.split(";")[0].split()[-1].split("[")[0] for ln in body.splitlines()[1:] if ";" in ln]
    assert names == list(DR.DECODE_DTYPE.names)
    assert DR.DECODE_DTYPE.itemsize == 40 and DR.DECODE_DTYPE.fields["dmin"][1] == 32 and DR.DECODE_DTYPE.fields["ndup"][1] == 38
    from cwsl_digi_amd import api
    assert api.DECODE_DTYPE == DR.DECODE_DTYPE


def test_bp_beats_osd_on_one_entry():
    msg, osd = _ft8([_msg(11, 4)], [_osd(22, 1, 3.5)])
    recs, n = DR.decodes("FT8", [(7, _where(1), msg, osd)])
    assert n == 1 and _rows(recs) == [(7, 0, 0, 0, 11, 4, 1)]
    assert recs[0]["dmin"].tobytes() == np.float32(0.0).tobytes()
    assert (recs[0]["freq_hz"], recs[0]["dt_s"], recs[0]["sync"]) == tuple(np.float32(v) for v in _where(1)[0])


def test_osd_word_only_when_osd_is_used():
    msg, osd = _ft8([_msg(None), _msg(12, 2)], [_osd(21, 30, 9.25), _osd(None)])
    recs, n = DR.decodes("FT8", [(0, _where(2), msg, osd)])
    assert _rows(recs) == [(0, 0, 1, 0, 21, 30, 1), (0, 1, 0, 0, 12, 2, 1)] and recs[0]["dmin"] == np.float32(9.25)
    recs, n = DR.decodes("FT8", [(0, _where(2), msg, None)])
    assert n == 1 and _rows(recs) == [(0, 1, 0, 0, 12, 2, 1)]


def test_all_zero_word_is_dropped():
    msg, osd = _ft8([_msg(0), _msg(None), _msg(5)], [_osd(None), _osd(0), _osd(None)])
    recs, n = DR.decodes("FT8", [(3, _where(3), msg, osd)])
    assert _rows(recs) == [(3, 2, 0, 0, 5, 0, 1)]
    assert DR.all_zero_word(_bits(0)) and not DR.all_zero_word(_bits(1))
    pad = np.zeros(12, np.uint8)
    pad[11] = 0x1F                                                      # the five padding bits are not part of the word
    assert DR.all_zero_word(pad)


def test_representative_by_osd_then_nharderr_then_entry():
    # word 9: OSD entry 0 with nharderr 0, BP entries 2 (nharderr 5) and 4 (nharderr 3): BP wins over OSD, then the fewer hard errors -> entry 4
    # word 8: BP entries 1 and 3, both nharderr 2: the tie on (by_osd, nharderr) goes to the smaller entry -> entry 1
    # word 6: OSD entries 5 (nharderr 20) and 6 (nharderr 20): -> entry 5;  word 4: OSD entries 7 (nharderr 31) and 8 (nharderr 30) -> entry 8
    msgs = [_msg(None), _msg(8, 2), _msg(9, 5), _msg(8, 2), _msg(9, 3), _msg(None), _msg(None), _msg(None), _msg(None)]
    osds = [_osd(9, 0, 1.0), _osd(None), _osd(None), _osd(None), _osd(None), _osd(6, 20, 2.0), _osd(6, 20, 2.5), _osd(4, 31, 3.0), _osd(4, 30, 4.0)]
    msg, osd = _ft8(msgs, osds)
    recs, n = DR.decodes("FT8", [(1, _where(9), msg, osd)])
    assert n == 4
    assert _rows(recs) == [(1, 1, 0, 0, 8, 2, 2), (1, 4, 0, 0, 9, 3, 3), (1, 5, 1, 0, 6, 20, 2), (1, 8, 1, 0, 4, 30, 2)]
    assert [float(r["dmin"]) for r in recs] == [0.0, 0.0, 2.0, 4.0]
    assert [float(r["freq_hz"]) for r in recs] == [101.0, 104.0, 105.0, 108.0]


def test_ndup_counts_every_carrier():
    msg, osd = _ft8([_msg(3, q % 4) for q in range(10)] + [_msg(None)], [_osd(None)] * 10 + [_osd(3, 40, 1.0)])
    recs, n = DR.decodes("FT8", [(0, _where(11), msg, osd)])
    assert _rows(recs) == [(0, 0, 0, 0, 3, 0, 11)]
    recs, n = DR.decodes("FT8", [(0, _where(11), msg, None)])
    assert _rows(recs) == [(0, 0, 0, 0, 3, 0, 10)]


def _ft4(entries):
    """entries: per record ((bp words), (osd words)) with None for a set without a word, nharderr = 10 * set + entry."""
    msg, osd = np.zeros(len(entries), D4.MSG4_DTYPE), np.zeros(len(entries), X4.OSD4_DTYPE)
    for q, (bp, od) in enumerate(entries):
        for s in range(3):
            msg["set"][q, s] = _msg(bp[s], 10 * s + q)
            osd["set"][q, s] = _osd(od[s], 10 * s + q, 1.0 + s)
    return msg, osd


def test_ft4_set_choice():
    N = (None, None, None)
    entries = [((None, 31, 32), (40, None, None)),      # BP set 1 before BP set 2 and before any OSD word
               (N, (None, None, 41)),                   # OSD only, set 2
               (N, (None, 42, 43)),                     # OSD only: the smallest set
               (N, N),                                  # nothing
               ((33, None, None), N)]
    msg, osd = _ft4(entries)
    recs, n = DR.decodes("FT4", [(2, _where(5), msg, osd)])
    assert _rows(recs) == [(2, 0, 0, 1, 31, 10, 1), (2, 1, 1, 2, 41, 21, 1), (2, 2, 1, 1, 42, 12, 1), (2, 4, 0, 0, 33, 4, 1)]
    assert [float(r["dmin"]) for r in recs] == [0.0, 3.0, 2.0, 0.0]
    recs, n = DR.decodes("FT4", [(2, _where(5), msg, None)])
    assert _rows(recs) == [(2, 0, 0, 1, 31, 10, 1), (2, 4, 0, 0, 33, 4, 1)]


def test_ft4_entry_is_the_compacted_index():
    """nrec 0, 1, 3 over three candidates: four records; the entry is the index as cwslg_fetch_ft4_sync compacts them (candidate order, then
    segment order), which is the index of the fetched arrays -- candidate 0 has none, candidate 1 gives entry 0, candidate 2 entries 1..3."""
    nrec = [0, 1, 3]
    recs4 = [dict(f0_hz=500.0 + 100 * k, f1_hz=501.0 + 100 * k + r, dt_s=0.1 * r, sync=3.0 + k, ibest=0, idf=0, seg=r + 1, cand=k)
             for k, m in enumerate(nrec) for r in range(m)]
    assert [r["cand"] for r in recs4] == [1, 2, 2, 2]
    N = (None, None, None)
    msg, osd = _ft4([((50, None, None), N), (N, N), ((None, None, 50), N), ((51, None, None), N)])
    recs, n = DR.decodes("FT4", [(0, DR.where_ft4(recs4), msg, osd)])
    # word 50: entries 0 (set 0, nharderr 0) and 2 (set 2, nharderr 22) -> entry 0, ndup 2
    assert _rows(recs) == [(0, 0, 0, 0, 50, 0, 2), (0, 3, 0, 0, 51, 3, 1)]
    assert float(recs[0]["freq_hz"]) == 601.0 and float(recs[1]["freq_hz"]) == 703.0 and float(recs[1]["dt_s"]) == np.float32(0.2)


def test_order_across_channels_and_no_dedup_between_them():
    a = _ft8([_msg(7, 1), _msg(6, 0)])
    b = _ft8([_msg(6, 0), _msg(None), _msg(7, 0)])
    empty = _ft8([])
    chans = [(9, _where(2), a[0], None), (2, _where(3), b[0], None), (5, [], empty[0], None)]
    recs, n = DR.decodes("FT8", chans)
    assert n == 4 and _rows(recs) == [(2, 0, 0, 0, 6, 0, 1), (2, 2, 0, 0, 7, 0, 1), (9, 0, 0, 0, 7, 1, 1), (9, 1, 0, 0, 6, 0, 1)]


def test_truncation_by_max():
    msg, _ = _ft8([_msg(20 + q, q) for q in range(5)])
    chans = [(0, _where(5), msg, None), (1, _where(5), msg, None)]
    full, n = DR.decodes("FT8", chans)
    assert n == 10 and len(full) == 10
    for m in (0, 1, 9, 10, 11):
        recs, n = DR.decodes("FT8", chans, m)
        assert n == 10 and recs.tobytes() == full[:min(m, 10)].tobytes()
    recs, n = DR.decodes("FT8", [], 5)
    assert n == 0 and len(recs) == 0
