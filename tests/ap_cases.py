"""Test helper: the inputs the a-priori tests share -- hand-made metric sets with their patterns (one per rule of the contract, the answers are
written out in tests/test_ap_ref.py), the mixed batch of the kernel test with its reference records, and the recipe of the GPU slots of the fetch
test.  Codes are made from a seed as in ldpc_cases; tests/test_ap_inputs.py vets with the restatements alone that every input is what it is for."""
import functools

import numpy as np

import ap_ref as AP
import ldpc_cases as LC
import ldpc_ref as R

F32 = np.float32
N, K = R.N, R.K
SEED = LC.SEEDS[0]
MAX_ITER = 30
NPRE = 29                                   # the known field of the patterns: codeword bits 0..28


def prefix_pattern(bits, n=NPRE):
    """(mask, value) over the first n positions with the given bits."""
    return (np.ones(n, np.uint8), np.asarray(bits[:n], np.uint8))


def message(mseed, prefix=None):
    """77 bits from the seed (the first len(prefix) replaced) + CRC-14."""
    b = np.random.default_rng(mseed).integers(0, 2, 77).astype(np.uint8)
    if prefix is not None:
        b[:len(prefix)] = prefix
    crc = R.crc14(b)
    return np.concatenate([b, [(crc >> (13 - i)) & 1 for i in range(14)]]).astype(np.uint8)


def noisy(seed, m91, noise, nseed):
    """llr = 2.83 (s + noise N(0, 1)), s = +-1 the codeword of m91 under the code of `seed` (ldpc_cases' scaling)."""
    cw = LC.encode(seed, m91)
    rng = np.random.default_rng(77000 + nseed)
    return (2.83 * ((2.0 * cw - 1.0) + noise * rng.standard_normal(N))).astype(F32)


PREFIXES = [np.random.default_rng(5100 + i).integers(0, 2, NPRE).astype(np.uint8) for i in range(8)]
PREFIXES[3] = np.zeros(NPRE, np.uint8)      # one known field of zeros (with an empty mask beside it: the plain second pass)


def patterns(n_pat):
    """The first n_pat of the eight patterns of the batch tests: known fields PREFIXES[i] over bits 0..28, pattern 5 an EMPTY mask."""
    pairs = [prefix_pattern(PREFIXES[i]) for i in range(n_pat)]
    if n_pat > 5:
        pairs[5] = (np.zeros(0, np.uint8), np.zeros(0, np.uint8))
    return AP.make_patterns(pairs)


# ---- the mixed batch of the kernel test -----------------------------------------------------------------------------------------------------
BATCH_N = 257
BATCH_SIZES = (0, 1, 3, 4, 5, 63, 64, 65, 257)
BATCH_NPAT = (1, 2, 8)
BATCH_NOISE = (0.62, 0.8, 0.9, 1.0)         # around and beyond BP's 50 % point under these codes


@functools.lru_cache(maxsize=None)
def batch(seed=SEED):
    """-> (llr float32[257, 174], sent: the 91 bits of a set that carries a transmission, else None).  Transmissions whose first 29 bits are one
    of the eight known fields at four noise levels, others with a random field, noise alone, signs, zeros, and two sets that are not finite."""
    rng = np.random.default_rng(31337)
    llr, sent = [], []
    for q in range(BATCH_N):
        kind = q % 16
        if kind == 13:
            x, m = (F32(2.83) * rng.standard_normal(N)).astype(F32), None
        elif kind == 14:
            x, m = (F32(3) * (2 * rng.integers(0, 2, N) - 1)).astype(F32), None
        elif kind == 15 and q < 64:
            x, m = np.zeros(N, F32), None
        else:
            m = message(9000 + q, PREFIXES[q % 8] if kind < 12 else None)
            x = noisy(seed, m, BATCH_NOISE[(q // 16) % 4], q)
        llr.append(x)
        sent.append(m)
    llr = np.stack(llr)
    llr[100, 17] = np.nan
    llr[201, 173] = -np.inf
    sent[100] = sent[201] = None
    llr.setflags(write=False)
    return llr, sent


@functools.lru_cache(maxsize=None)
def batch_reference(n_pat, seed=SEED):
    """The restatement's records of batch(seed) under patterns(n_pat): computed once, shared by the tests."""
    rec = AP.decode(LC.make_code(seed)["code"], batch(seed)[0], patterns(n_pat), MAX_ITER)
    rec.setflags(write=False)
    return rec


# ---- hand-made sets, one per rule (the answers: tests/test_ap_ref.py) ------------------------------------------------------------------------
def _clean(m91, amp=2.83, seed=SEED):
    return (amp * (2.0 * LC.encode(seed, m91) - 1.0)).astype(F32)


@functools.lru_cache(maxsize=None)
def rule_cases(seed=SEED):
    """-> {name: (patterns PATTERN_DTYPE[], llr float32[174], the word the case is about (91 bits) or None)}."""
    out = {}
    m = message(4001, PREFIXES[0])
    right, wrong = prefix_pattern(m), prefix_pattern(1 - m)
    x = _clean(m)
    x[40] = np.nan
    out["nan"] = (AP.make_patterns([right]), x, None)
    x = _clean(m)
    x[173] = np.inf
    out["inf"] = (AP.make_patterns([right]), x, None)
    out["zeros"] = (AP.make_patterns([right]), np.zeros(N, F32), None)                       # A = 0: the forced bits are +-0, z > 0 is false
    out["zeros_zero_value"] = (AP.make_patterns([prefix_pattern(np.zeros(NPRE))]), np.zeros(N, F32), np.zeros(K, np.uint8))
    empty = (np.zeros(0, np.uint8), np.zeros(0, np.uint8))
    out["empty_mask_clean"] = (AP.make_patterns([empty]), noisy(seed, m, 0.45, 1), m)
    out["empty_mask_noise"] = (AP.make_patterns([empty]), (F32(2.83) * np.random.default_rng(8).standard_normal(N)).astype(F32), None)
    out["all77"] = (AP.make_patterns([(np.ones(77, np.uint8), m[:77])]), noisy(seed, m, 1.2, 2), m)
    out["second_right"] = (AP.make_patterns([wrong, right]), noisy(seed, m, 0.8, NOISY_SEED), m)
    out["no_success"] = (AP.make_patterns([wrong, prefix_pattern(PREFIXES[1]), prefix_pattern(PREFIXES[2])]), noisy(seed, m, 0.8, NOISY_SEED), None)
    # a clean codeword whose bit 3 the channel contradicts (-+5 against the +-2.83 of the rest); the pattern holds the right bit
    x = _clean(m)
    x[3] = F32(-5.0) if m[3] else F32(5.0)
    out["original_metrics"] = (AP.make_patterns([right]), x, m)
    # strong metrics for a codeword that disagrees with the pattern in one bit: the loop returns to the codeword, the rule rejects it
    v = m.copy()
    v[5] ^= 1
    out["contradicts"] = (AP.make_patterns([prefix_pattern(v)]), _clean(m, 10.0), m)
    for pat, x, w in out.values():
        x.setflags(write=False)
    return out


NOISY_SEED = 4          # test_ap_inputs.py: under this seed BP and OSD order 2 both miss the word at noise 0.8 and pattern `right` finds it


# ---- the GPU slots of the fetch test ---------------------------------------------------------------------------------------------------------
# One slot of IQ at 48 kHz on one receiver, five FT8 channels (record_race_cases' noise, sync and decode settings, harvest_cases' syncmin):
#   channel 0  a strong transmission of message A (BP decodes it) and weak ones in the range BP and OSD fail on (SLOT_TX below);
#   channel 1  a strong transmission whose field no pattern holds: decodes, no a-priori find;
#   channels 2..4  noise alone: a run of channels without finds.
# tests/test_ap_inputs.py proves on the CPU chain what the slot contains.
import decodes_ref as DR                     # noqa: E402
import ft8_softbits_ref as S8                # noqa: E402
import osd_cases as OC                       # noqa: E402
import osd_ref as O                          # noqa: E402
import record_race_cases as RC               # noqa: E402

FS, BLK8 = RC.FS, RC.BLK["FT8"]
SLOT_RF = (RC.RF["FT8"][0], RC.RF["FT8"][1], 2000, 6000, -9000)
SLOT_SYNC = dict(RC.SYNC, syncmin=1.2)
SLOT_MAX_CAND = 100
SLOT_MIN_NSYNC = 7
STRONG, WEAK = 2500.0, 700.0
MSG_A, MSG_B, MSG_C, MSG_D, MSG_E = (message(6001, PREFIXES[0]), message(6002, PREFIXES[0]), message(6003, PREFIXES[1]), message(6004),
                                     message(6005, PREFIXES[1]))
# (audio Hz of tone 0, start s, amplitude, message); the weak levels were searched on the CPU chain -- what each gives is test_ap_inputs.py's to prove:
#   A strong: BP.  A weak: BP and OSD fail, pattern 0 finds it -- the word a BP record of another entry carries.  B twice at 900: BP on one, OSD
#   alone on the other (with OSD off at the boundary that entry is attempted and pattern 0 finds it: the gate changes).  C: pattern 1.  E twice:
#   pattern 1 on two entries, one decode with ndup 2.
SLOT_TX = {0: [(3.125 * 160, 0.04 * 8, STRONG, MSG_A), (3.125 * 400, 0.04 * 12, WEAK, MSG_A), (3.125 * 320, 0.04 * 20, 900.0, MSG_B),
               (3.125 * 672, 0.04 * 20, 900.0, MSG_B), (3.125 * 860, 0.04 * 15, WEAK, MSG_C), (3.125 * 520, 0.04 * 25, 950.0, MSG_E),
               (3.125 * 760, 0.04 * 25, 950.0, MSG_E)],
           1: [(3.125 * 300, 0.04 * 10, STRONG, MSG_D)]}
start_epoch = lambda e: RC.start_epoch("FT8", e)


def slot_patterns(n_pat=2):
    return patterns(n_pat)


def bits12(m91):
    return np.packbits(np.concatenate([m91, np.zeros(5, np.uint8)])).tobytes()


@functools.lru_cache(maxsize=None)
def slot_iq(seed=SEED):
    n, sigma = RC.N_IQ["FT8"], RC.SIGMA["FT8"]
    rng = np.random.default_rng(2)
    iq = (rng.normal(0.0, sigma, n) + 1j * rng.normal(0.0, sigma, n)).astype(np.complex64)
    for k, txs in SLOT_TX.items():
        for audio, t0, amp, m in txs:
            iq = iq + LC.iq_of_tones(FS, n, SLOT_RF[k], audio, t0, amp, LC.tones_of(LC.encode(seed, m)))
    iq = iq.astype(np.complex64)
    iq.setflags(write=False)
    return iq


@functools.lru_cache(maxsize=None)
def slot_chain(k, max_cand=SLOT_MAX_CAND, seed=SEED):
    """Every stage of channel k of the slot on the CPU: list, soft bits, decode and OSD records (harvest_cases' chain), then the a-priori records
    under slot_patterns() behind the fetch's gate, with OSD used and not used."""
    from oracle import oracle as orc
    oc = orc.Channel("FT8", FS, BLK8, SLOT_RF[k])
    assert oc.boundary(start_epoch(0)) is None
    oc.push_many(slot_iq(seed))
    fr = oc.boundary(start_epoch(1))["i16"]
    oc.close()
    code, G = LC.make_code(seed)["code"], OC.generator(seed)
    cands = orc.ft8_sync(fr, SLOT_SYNC["f_lo"], SLOT_SYNC["f_hi"], SLOT_SYNC["syncmin"], max_cand)
    llr, sigma, nsync = S8.softbits(orc.ft8_spectra(fr, S8.soft_pitch(SLOT_SYNC["f_hi"])), cands)
    msg = R.hard_records(code, llr, RC.DECODE8[0], nsync, sigma, RC.DECODE8[1])
    osd = O.chain_records(G, llr, RC.OSD8[0], nsync, msg, RC.OSD8[1])
    out = dict(list=cands, soft=(llr, sigma, nsync), msg=msg, osd=osd)
    for name, o in (("ap", osd), ("ap_no_osd", None)):
        out[name] = AP.decode(code, llr, slot_patterns(), MAX_ITER, AP.fetch_gate(msg, o, nsync, SLOT_MIN_NSYNC)) if len(llr) else np.zeros(0, AP.AP_MSG_DTYPE)
    return out


def ap_decodes(channels, max_out=None):
    """What cwslg_fetch_ft8_ap hands out.  channels: [(ch_id, where, ap records AP_MSG_DTYPE)] of the channels that take part: decodes_ref on the
    a-priori records in the decode records' place and no OSD records, then by_osd = 2, set = the pattern, dmin = the a-priori record's."""
    rec, n_total = DR.decodes("FT8", [(c, w, a["msg"], None) for c, w, a in channels], max_out)
    by_ch = {c: a for c, w, a in channels}
    for r in rec:
        a = by_ch[int(r["ch_id"])][int(r["entry"])]
        r["by_osd"], r["set"], r["dmin"] = 2, a["msg"]["pad_"], a["dmin"]
    return rec, n_total
