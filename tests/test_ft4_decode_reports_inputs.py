"""CPU: the slots of tests/ft4_decode_report_cases.py contain what tests/test_gpu_ft4_decode_reports.py needs them to contain -- proved with the
restatements alone, on the CPU oracle's frames -- and the physics of the restatement: on frequency, in white noise, the reported dB follows the
injected SNR."""
import numpy as np

import ft4_decode_report_cases as D
import ft4_decode_reports_ref as R4
import harvest_twin_cases as T

# Measured here, on the CPU, with the restatement (ft4_decode_report_cases.physics: 16 on-frequency transmissions, four levels 6.02 dB apart;
# DESIGN.md 4.11): reported snr_db - injected SNR in 2500 Hz = +0.06 dB on average, between -1.38 and +0.87 dB, standard deviation 0.59 dB: a
# spread of 1.44 dB around the mean.  Nobody has measured the figure before and it has never been compared with jt9's.
OFFSET_DB, SPREAD_DB = 0.06, 1.44


def _all():
    """[(slot, decode, report, sync record, (audio Hz, start s) of the transmission that carries the word, or None)]"""
    out = []
    for e in range(D.N_EPOCHS):
        dec, rep = D.expected(e)
        sent = {T.sent_bits(m): (a, t0) for a, t0, _, m, *_ in tuple(T.TRANSMISSIONS[e]) + tuple(D.extra_transmissions(e))}
        for d, r in zip(dec, rep):
            out.append((e, d, r, D.chain(int(d["ch_id"]), e)["sync"][int(d["entry"])], sent.get(bytes(d["bits"]))))
    return out


def test_the_slots_contain_what_the_gpu_tests_need():
    rows = _all()
    assert any(d["by_osd"] == 0 for _, d, _, _, _ in rows)                                  # a decode by BP
    assert any(d["by_osd"] == 1 for _, d, _, _, _ in rows)                                  # a decode by OSD alone
    assert max(d["ndup"] for _, d, _, _, _ in rows) >= 3 and any(d["set"] != 0 for _, d, _, _, _ in rows)
    floor = 0
    for e in range(D.N_EPOCHS):
        mine = [(d, r, s, tx) for ee, d, r, s, tx in rows if ee == e]
        early = [(r, s) for d, r, s, tx in mine if tx is not None and tx[1] == D.EARLY_T0]
        late = [(r, s) for d, r, s, tx in mine if tx is not None and tx[1] == D.LATE_T0]
        shadow = [(r, s) for d, r, s, tx in mine if tx is not None and tx[0] == D.shadowed_transmission(e)[0]]
        assert early and all(s["ibest"] < 0 for _, s in early)                              # its first symbols lie before sample 0
        assert late and all(s["ibest"] + 3296 > 4032 for _, s in late)                      # its last symbols fall beyond sample 4031
        assert all(r["nsync"] < 16 for r, _ in late + early)                                # (so Costas symbols are missing)
        assert shadow and all(r["xnoise"] > 0.4 * r["xsig"] and r["nsymerr"] == 0 and r["snr_db"] < -20.9 for r, _ in shadow)
        floor += sum(1 for r, _ in shadow if r["snr_db"] == -21)
    assert floor >= 1                                                                       # a decodable word whose report sits on the floor, not for want of power
    rep = np.array([r for _, _, r, _, _ in rows])
    assert (rep["nsymerr"] == 0).any() and (rep["nsymerr"] > 0).any()
    assert (rep["snr_db"] == -21).any() and (rep["snr_db"] > -21).any()
    assert (rep["snr_db"] >= -21).all() and (rep["nsync"] >= 0).all() and (rep["nsync"] <= 16).all() and (rep["nsymerr"] <= 87).all()
    # every decoded word that was sent re-encodes to the tones that were sent: the encoder is the inverse of the chain
    for e, d, _, _, tx in rows:
        if tx is not None:
            m = next(m for a, t0, _, m, *_ in tuple(T.TRANSMISSIONS[e]) + tuple(D.extra_transmissions(e)) if (a, t0) == tx)
            assert np.array_equal(R4.tones(D.K.encoder(D.SEED), d["bits"]), D.sent_tones(m))


def test_nsync_is_the_soft_records():
    for e in range(D.N_EPOCHS):
        dec, rep = D.expected(e)
        for d, r in zip(dec, rep):
            assert r["nsync"] == D.chain(int(d["ch_id"]), e)["soft"]["nsync"][int(d["entry"])]


def test_reported_db_follows_the_injected_snr():
    """Four injected levels 6.02 dB apart, four on-frequency transmissions each: snr_db rises monotonically at every frequency, and lies at the
    measured offset from the SNR in 2500 Hz within twice the observed spread.  The offset is a measurement, not part of the contract."""
    ph = D.physics()
    assert len(ph) == 16
    for hz in D.PHYS_HZ:
        got = [p[3] for p in ph if p[1] == hz]
        assert len(got) == 4 and all(x < y for x, y in zip(got, got[1:])), (hz, got)
    off = np.array([got - inj for _, _, inj, got, _ in ph])
    print(f"reported - injected: mean {off.mean():+.2f} dB, min {off.min():+.2f}, max {off.max():+.2f}, standard deviation {off.std():.2f} dB")
    for lv, hz, inj, got, nerr in ph:
        print(f"level {lv} {hz:.0f} Hz: injected {inj:+.2f} dB, reported {got:+.2f} dB, offset {got - inj:+.2f} dB, nsymerr {nerr}")
        assert got > -21.0
        assert abs(got - inj - OFFSET_DB) <= 2 * SPREAD_DB, (lv, hz, inj, got)
    steps = [np.mean([p[3] for p in ph if p[0] == lv + 1]) - np.mean([p[3] for p in ph if p[0] == lv]) for lv in range(3)]
    assert all(abs(s - 6.02) <= 2 * SPREAD_DB for s in steps), steps
