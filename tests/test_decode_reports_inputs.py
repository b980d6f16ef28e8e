"""CPU: the slots of tests/decode_report_cases.py contain what tests/test_gpu_decode_reports.py needs them to contain -- proved with the
restatements alone, on the CPU oracle's frames -- and the physics of the restatement: on the grid, in white noise, the reported dB follows the
injected SNR."""
import numpy as np

import decode_report_cases as D
import decode_reports_ref as RR
import harvest_cases as H

# Measured here, on the CPU, with the restatement (decode_report_cases.physics: 16 on-grid transmissions, four levels 6 dB apart):
# reported snr_db - injected SNR in 2500 Hz = -0.84 dB on average, between -1.34 and +0.19 dB: a spread of 1.04 dB around the mean.
OFFSET_DB, SPREAD_DB = -0.84, 1.04


def _all():
    """[(slot, decode, report, (freq_bin, time_step), (audio Hz, start s) of the transmission that carries the word, or None)]"""
    out = []
    for e in range(D.N_EPOCHS):
        dec, rep = D.expected(e)
        sent = {H.sent_bits(m): (a, t0) for a, t0, _, m in D.transmissions(e)}
        for d, r in zip(dec, rep):
            c = D.chain(int(d["ch_id"]), e)["list"][int(d["entry"])]
            out.append((e, d, r, (int(c[0]), int(c[1])), sent.get(bytes(d["bits"]))))
    return out


def test_the_slots_contain_what_the_gpu_tests_need():
    rows = _all()
    assert any(d["by_osd"] == 0 for _, d, _, _, _ in rows)                                  # a decode by BP
    assert any(d["by_osd"] == 1 for _, d, _, _, _ in rows)                                  # a decode by OSD alone
    assert any(d["ndup"] > 1 for _, d, _, _, _ in rows)                                     # a word on more than one list entry
    for e in range(D.N_EPOCHS):
        mine = [(d, r, ij, tx) for ee, d, r, ij, tx in rows if ee == e]
        late = [(r, ij) for d, r, ij, tx in mine if tx == (3.125 * 300, 0.04 * D.LATE_STEPS)]
        early = [(r, ij) for d, r, ij, tx in mine if tx == (3.125 * 600, 0.04 * D.EARLY_STEPS)]
        edge = [(r, ij) for d, r, ij, tx in mine if tx is not None and tx[0] == 3.125 * D.EDGE_BIN]
        shadow = [(r, ij) for d, r, ij, tx in mine if tx is not None and tx[0] == 3.125 * D.SHADOW_BIN]
        assert late and all(ij[1] + 12 + 4 * 78 > RR.NHSYM for _, ij in late)               # its last symbols fall beyond step 372
        assert early and all(ij[1] + 12 < 1 for _, ij in early)                             # its first symbols fall before step 1
        assert all(r["nsync"] < 21 for r, _ in late + early)                                # (so Costas symbols are missing)
        assert edge and all(ij[0] == D.EDGE_BIN and ij[0] + 14 > 960 for _, ij in edge)     # tone 7 lies above the band's last searched bin
        assert shadow and all(r["snr_db"] == -24 and r["xnoise"] > 0 for r, _ in shadow)    # clamped at -24 dB, and not for want of power
    rep = np.array([r for _, _, r, _, _ in rows])
    assert (rep["nsymerr"] == 0).any() and (rep["nsymerr"] > 0).any()
    assert (rep["snr_db"] == -24).any() and (rep["snr_db"] > -24).any()
    assert (rep["snr_db"] >= -24).all() and (rep["nsync"] >= 0).all() and (rep["nsync"] <= 21).all() and (rep["nsymerr"] <= 58).all()
    # every decoded word that was sent re-encodes to the tones that were sent: the encoder is the inverse of the chain
    for e, d, _, _, tx in rows:
        if tx is not None:
            m = next(m for a, t0, _, m in D.transmissions(e) if (a, t0) == tx)
            assert np.array_equal(RR.tones(D.K.encoder(D.SEED), d["bits"]), D.sent_tones(m))


def test_nsync_is_the_soft_records():
    for e in range(D.N_EPOCHS):
        dec, rep = D.expected(e)
        for d, r in zip(dec, rep):
            assert r["nsync"] == D.chain(int(d["ch_id"]), e)["soft"][2][int(d["entry"])]


def test_reported_db_follows_the_injected_snr():
    """Four injected levels 6 dB apart, four on-grid transmissions each: snr_db rises monotonically at every frequency, and lies at the measured
    offset from the SNR in 2500 Hz within twice the observed spread.  The offset is a measurement, not part of the contract."""
    ph = D.physics()
    assert len(ph) == 16
    for b in D.PHYS_BINS:
        got = [p[3] for p in ph if p[1] == b]
        assert len(got) == 4 and all(x < y for x, y in zip(got, got[1:])), (b, got)
    for lv, b, inj, got, _ in ph:
        print(f"level {lv} bin {b}: injected {inj:+.2f} dB, reported {got:+.2f} dB, offset {got - inj:+.2f} dB")
        assert got > -24.0
        assert abs(got - inj - OFFSET_DB) <= 2 * SPREAD_DB, (lv, b, inj, got)
    steps = [np.mean([p[3] for p in ph if p[0] == lv + 1]) - np.mean([p[3] for p in ph if p[0] == lv]) for lv in range(3)]
    assert all(abs(s - 6.02) <= 2 * SPREAD_DB for s in steps), steps
