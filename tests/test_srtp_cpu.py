"""CPU: SRTP packet protection (hilcodec_amd/srtp.py, the definition of hilc_srtp_protect and hilc_srtp_unprotect): the row layouts
against the C header, the published known answers of every primitive (FIPS 197 C.1, RFC 3711 B.2 and B.3) and of whole packets, the
model's HMAC against the standard library's, and SenderModel / ReceiverModel on scripted traces: round trip, forgeries, replays, the
window's edge, the rollover on both sides, a late joiner, and the rules that keep a keystream from being used twice.  Everything is
integer: every comparison is exact."""
import hashlib
import hmac
import os
import re

import numpy as np
import pytest

from hilcodec_amd import forward, srtp, wire
from tests.hops import HEADER, assert_entry_points

H = bytes.fromhex
MASTER_KEY, MASTER_SALT = H("E1F97A0D3E018BE0D64FA32C06DE4139"), H("0EC675AD498AFEEBB6960B3AABE6")
K_E, K_S = H("C61E7A93744F39EE10734AFE3FF7A087"), H("30CBBC08863D8C85D49DB34A9AE1")
K_A = H("CEBE321F6FF7716B6FD4AB49AF256A156D38BAA4")
TB = 40


# ---------------------------------------------------------------- layout and entry points
def test_layouts_match_header():
    """srtp.<NAME> is `#define HILC_SRTP_<NAME>`, value for value; the rows are dense and the names are the counters"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    env, header = {}, {}
    for name, expr in re.findall(r"^#define (HILC_\w+)[ \t]+(\S.*?)[ \t]*$", text, re.M):
        env[name] = eval(re.sub(r"\b(0x[0-9A-Fa-f]+|\d+)[uU]\b", r"\1", expr), {"__builtins__": {}}, env)
        if name.startswith("HILC_SRTP_"):
            header[name[len("HILC_SRTP_"):]] = env[name]
    host_only = {"TAG_BYTES", "KEY_BYTES", "SALT_BYTES", "AUTH_BYTES"}
    python = {k: v for k, v in vars(srtp).items() if k.isupper() and isinstance(v, int) and not isinstance(v, bool) and k not in host_only}
    assert len(header) == 27 and header == python
    assert env["HILC_WIRE_SRTP_TAG_BYTES"] == wire.SRTP_TAG_BYTES == srtp.TAG_BYTES == 10
    assert wire.srtp_bytes(8, 2, 3) == wire.transport_bytes(8, 2, 3) + 10
    assert (srtp.KEY_RK, srtp.KEY_SALT, srtp.KEY_INNER, srtp.KEY_OUTER, srtp.KEY_WORDS) == (3, 47, 51, 56, 61)
    assert sorted(v for k, v in header.items() if k.startswith("TX_") and k != "TX_WORDS") == list(range(srtp.TX_WORDS))
    assert sorted(v for k, v in header.items() if k.startswith("RX_") and k != "RX_WORDS") == list(range(srtp.RX_WORDS))
    assert [getattr(srtp, "TX_" + n.upper()) for n in srtp.TX_NAMES] == list(range(srtp.TX_PROTECTED, srtp.TX_WORDS))
    assert [getattr(srtp, "RX_" + n.upper()) for n in srtp.RX_NAMES] == list(range(srtp.RX_OK, srtp.RX_WORDS))


def test_entry_points_are_declared_exported_and_bound():
    assert_entry_points(("hilc_srtp_protect", "hilc_srtp_unprotect"), in_abi16_line=True)
    assert os.path.isfile(os.path.join(os.path.dirname(srtp.__file__), "csrc", "srtp.hip"))
    import hilcodec_amd
    assert callable(hilcodec_amd.srtp_protect) and callable(hilcodec_amd.srtp_unprotect)


# ---------------------------------------------------------------- known answers
def test_aes128_fips197_c1():
    assert srtp.aes_encrypt(bytes(range(16)), H("00112233445566778899aabbccddeeff")) == H("69c4e0d86a7b0430d8cdb78070b4c55a")
    assert srtp.SBOX[0x00] == 0x63 and srtp.SBOX[0x53] == 0xED and sorted(srtp.SBOX) == list(range(256))
    assert srtp.TE0[0] == 0xC66363A5 and srtp.TE0[255] == 0x2C16163A


def test_aes_cm_keystream_rfc3711_b2():
    ks = srtp.aes_cm_keystream(H("2B7E151628AED2A6ABF7158809CF4F3C"), H("F0F1F2F3F4F5F6F7F8F9FAFBFCFD"), 0, 0, 48)
    assert ks == H("e03ead0935c95e80e166b16dd92b4eb4" "d23513162b02d0f72a43a2fe4a5f97ab" "41e95b3bb0a2e8dd477901e4fca894c0")
    assert srtp.aes_cm_keystream(H("2B7E151628AED2A6ABF7158809CF4F3C"), H("F0F1F2F3F4F5F6F7F8F9FAFBFCFD"), 0, 0, 17) == ks[:17]


def test_key_derivation_rfc3711_b3():
    assert srtp.derive(MASTER_KEY, MASTER_SALT) == (K_E, K_A, K_S)
    row = srtp.key_row(MASTER_KEY, MASTER_SALT, 0xCAFEBABE, roc=3)
    assert row.dtype == np.int32 and row.shape == (srtp.KEY_WORDS,) and row[srtp.KEY_VALID] == 1 and row[srtp.KEY_ROC] == 3
    assert int(row[srtp.KEY_SSRC]) & 0xFFFFFFFF == 0xCAFEBABE
    assert np.array_equal(row, srtp.session_key_row(K_E, K_A, K_S, 0xCAFEBABE, 3))
    salt = b"".join((int(w) & 0xFFFFFFFF).to_bytes(4, "big") for w in row[srtp.KEY_SALT:srtp.KEY_SALT + 4])
    assert salt == K_S + b"\0\0"
    assert [int(w) & 0xFFFFFFFF for w in row[srtp.KEY_RK:srtp.KEY_RK + 4]] == [int.from_bytes(K_E[4 * i:4 * i + 4], "big") for i in range(4)]


@pytest.mark.parametrize("ssrc, roc, seq, flags, body, want", [
    (0xCAFEBABE, 0, 0x1234, 0x08, bytes(range(10)), "123408e5ff75e44837d5742f06a9d11d30e4b1954c8eca"),
    (0xCAFEBABE, 1, 0x0001, 0x48, bytes(range(0x10, 0x1D)), "0001480d4b491ce71c85108e9de41cd21bf93e9df9d65357f277"),
    (0, 0, 0, 0x80, bytes(range(1, 40)),
     "000080fb61bf426d6e5c6df1f017ef9d92e5c55ce916e541a034c5fba126cb0ac1dcdbd42cdf43fd318d0a12f828e5055593a357"),
])
def test_whole_packets(ssrc, roc, seq, flags, body, want):
    row = srtp.session_key_row(K_E, K_A, K_S, ssrc)
    plain = bytes([seq >> 8, seq & 255, flags]) + body
    got = srtp.protect_packet(row, plain, roc)
    assert got == H(want) and len(got) == len(plain) + 10
    if seq == 0x1234:
        iv = srtp._iv(srtp._salt_words(K_S), ssrc, roc, seq)
        assert b"".join(w.to_bytes(4, "big") for w in iv) == H("30cbbc084cc3363bd49db34a88d50000")
    # the receiver's side of the same vector, from a row at the packet's own ROC
    rx = np.zeros(srtp.RX_WORDS, dtype=np.int32)
    rx[srtp.RX_ROC] = roc
    assert srtp.unprotect_packet(row, rx, got, len(got), len(plain)) == plain and rx[srtp.RX_OK] == 1


def test_hmac_equals_the_standard_library():
    rng = np.random.default_rng(5)
    inner, outer = srtp.hmac_midstates(K_A)
    for n in range(131):
        msg = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert srtp.hmac_sha1_mid(inner, outer, msg) == hmac.new(K_A, msg, hashlib.sha1).digest(), n
    assert srtp.hmac_sha1(b"", b"") == hmac.new(b"", b"", hashlib.sha1).digest()


# ---------------------------------------------------------------- traces
def _pair(batch=2, roc=0):
    tx, rx = srtp.SenderModel(batch, TB), srtp.ReceiverModel(batch, TB)
    for b in range(batch):
        key, salt = bytes([b + 1]) * 16, bytes([b + 9]) * 14
        tx.keys.set_key(b, key, salt, ssrc=100 + b, roc=roc)
        rx.keys.set_key(b, key, salt, ssrc=100 + b, roc=roc)
    start = np.ones(batch, dtype=np.int32)
    tx.protect(np.zeros((batch, TB), dtype=np.uint8), np.zeros(batch, dtype=np.int32), start)
    rx.start(start)
    return tx, rx


def _send(tx, slot, seq, body=b"\x11\x22\x33\x44\x55"):
    """one headed packet of `slot` through the sender model -> the protected bytes"""
    plain = wire.pack_transport(seq, body, 1)
    packets = np.zeros((tx.B, TB), dtype=np.uint8)
    nbytes = np.zeros(tx.B, dtype=np.int32)
    packets[slot, :len(plain)] = np.frombuffer(plain, dtype=np.uint8)
    nbytes[slot] = len(plain)
    out = tx.protect(packets, nbytes)
    assert out["nbytes"][slot] == len(plain) + 10 and not out["packets"][slot, len(plain) + 10:].any()
    other = [b for b in range(tx.B) if b != slot]
    assert not out["nbytes"][other].any() and not out["packets"][other].any()
    return plain, out["packets"][slot, :len(plain) + 10].tobytes()


def test_round_trip_and_independent_slots():
    tx, rx = _pair()
    for seq in range(5):
        for slot in (0, 1):
            plain, prot = _send(tx, slot, seq, bytes([seq, slot, 7]))
            assert prot[:3] == plain[:3] and prot[3:len(plain)] != plain[3:]
            assert rx.push(slot, prot) == plain
    assert rx.state[:, srtp.RX_OK].tolist() == [5, 5] and tx.state[:, srtp.TX_PROTECTED].tolist() == [5, 5]
    assert rx.state[:, srtp.RX_SL].tolist() == [4, 4] and rx.state[0, srtp.RX_WIN_LO] == 0b11111
    plain, prot = _send(tx, 0, 5)
    assert rx.push(1, prot) is None and rx.state[1, srtp.RX_AUTH_FAIL] == 1          # another slot's key


def test_every_flipped_bit_is_an_auth_fail_that_leaves_the_row():
    tx, rx = _pair(1)
    _, first = _send(tx, 0, 0)
    assert rx.push(0, first) is not None
    plain, prot = _send(tx, 0, 1)
    fails = 0
    for bit in range(8 * len(prot)):
        before = rx.state.copy()
        forged = bytearray(prot)
        forged[bit >> 3] ^= 1 << (bit & 7)
        assert rx.push(0, bytes(forged)) is None, bit
        fails += 1
        # a flipped SEQ bit may also land outside the window or on the packet already seen: a replay, never an acceptance
        changed = np.nonzero(rx.state[0] != before[0])[0].tolist()
        assert changed in ([srtp.RX_AUTH_FAIL], [srtp.RX_REPLAY]), (bit, changed)
        if bit >= 16:
            assert changed == [srtp.RX_AUTH_FAIL], bit
    assert rx.state[0, srtp.RX_AUTH_FAIL] + rx.state[0, srtp.RX_REPLAY] == fails
    assert rx.push(0, prot) == plain


def test_replay_reorder_and_the_window_edge():
    tx, rx = _pair(1)
    sent = {seq: _send(tx, 0, seq) for seq in range(70)}
    for seq in (0, 2, 1):                                    # a reorder inside the window
        assert rx.push(0, sent[seq][1]) == sent[seq][0]
    assert rx.state[0, srtp.RX_SL] == 2 and rx.state[0, srtp.RX_WIN_LO] == 0b111
    assert rx.push(0, sent[1][1]) is None and rx.push(0, sent[2][1]) is None and rx.state[0, srtp.RX_REPLAY] == 2
    assert rx.push(0, sent[69][1]) == sent[69][0]            # the window moves up by 67: everything before falls out
    assert rx.state[0, srtp.RX_WIN_LO] == 1 and rx.state[0, srtp.RX_WIN_HI] == 0
    assert rx.push(0, sent[6][1]) == sent[6][0]              # 63 below the highest: the window's last bit
    assert rx.state[0, srtp.RX_WIN_HI] == np.int32(-(1 << 31))
    assert rx.push(0, sent[5][1]) is None                    # 64 below: outside, whether it was seen or not
    assert rx.push(0, sent[6][1]) is None
    assert rx.state[0, srtp.RX_REPLAY] == 4 and rx.state[0, srtp.RX_OK] == 5 and rx.state[0, srtp.RX_AUTH_FAIL] == 0


def test_short_and_overlong_arrivals():
    tx, rx = _pair(1)
    _, prot = _send(tx, 0, 0)
    for cut in (0, 2, 12):
        assert rx.push(0, prot[:cut]) is None
    assert srtp.unprotect_packet(rx.keys.rows[0], rx.state[0], prot + bytes(60), TB + 11, TB) is None
    assert rx.state[0, srtp.RX_SHORT] == 4 and rx.state[0, srtp.RX_SEEN] == 0
    assert rx.push(0, prot[:13]) is None and rx.state[0, srtp.RX_AUTH_FAIL] == 1      # long enough to carry a tag: the tag decides


def test_rollover_on_both_sides():
    tx, rx = _pair(1)
    sent = {}
    for seq in (0xFFFD, 0xFFFE, 0xFFFF, 0x0000, 0x0001):
        sent[seq] = _send(tx, 0, seq)
    assert tx.state[0, srtp.TX_ROC] == 1 and tx.state[0, srtp.TX_LAST] == 1
    assert rx.push(0, sent[0xFFFD][1]) == sent[0xFFFD][0]
    for seq, roc_after, sl_after in ((0xFFFE, 0, 0xFFFE), (0x0000, 1, 0), (0xFFFF, 1, 0), (0x0001, 1, 1)):
        assert rx.push(0, sent[seq][1]) == sent[seq][0], hex(seq)           # FFFF arrives after the wrap: v = ROC - 1
        assert (rx.state[0, srtp.RX_ROC], rx.state[0, srtp.RX_SL]) == (roc_after, sl_after), hex(seq)
    assert rx.state[0, srtp.RX_OK] == 5 and rx.state[0, srtp.RX_WIN_LO] == 0b11111
    assert rx.push(0, sent[0xFFFF][1]) is None and rx.state[0, srtp.RX_REPLAY] == 1
    # the same bytes under the wrong rollover counter do not authenticate
    fresh = srtp.ReceiverModel(1, TB)
    fresh.keys.rows[0] = rx.keys.rows[0]
    assert fresh.push(0, sent[0x0001][1]) is None and fresh.state[0, srtp.RX_AUTH_FAIL] == 1


def test_an_early_packet_of_the_previous_cycle_is_a_replay_at_roc_0():
    tx, rx = _pair(1)
    plain, prot = _send(tx, 0, 3)
    assert rx.push(0, prot) == plain
    forged = bytes([0xFF, 0xF0]) + prot[2:]                  # SEQ - s_l > 32768 at ROC 0: v = -1
    assert rx.push(0, forged) is None and rx.state[0, srtp.RX_REPLAY] == 1 and rx.state[0, srtp.RX_AUTH_FAIL] == 0


def test_a_receiver_started_at_roc_3():
    tx, rx = _pair(1, roc=3)
    assert tx.state[0, srtp.TX_ROC] == 3 and rx.state[0, srtp.RX_ROC] == 3
    plain, prot = _send(tx, 0, 0x8000)
    late = srtp.ReceiverModel(1, TB)
    late.keys.set_key(0, bytes([1]) * 16, bytes([9]) * 14, ssrc=100)         # the same key at ROC 0
    late.start([1])
    assert late.push(0, prot) is None and late.state[0, srtp.RX_AUTH_FAIL] == 1
    assert rx.push(0, prot) == plain and rx.state[0, srtp.RX_ROC] == 3
    assert prot == srtp.protect_packet(rx.keys.rows[0], plain, 3) != srtp.protect_packet(rx.keys.rows[0], plain, 0)


def test_a_slot_without_a_key_sends_and_accepts_nothing():
    tx, rx = _pair(2)
    _, prot = _send(tx, 1, 0)
    tx.keys.clear_key(1)
    rx.keys.clear_key(1)
    plain = wire.pack_transport(1, b"\1\2\3\4\5", 1)
    packets = np.zeros((2, TB), dtype=np.uint8)
    packets[:, :len(plain)] = np.frombuffer(plain, dtype=np.uint8)
    out = tx.protect(packets, [len(plain), len(plain)])
    assert out["nbytes"].tolist() == [len(plain) + 10, 0] and not out["packets"][1].any()
    assert tx.state[1, srtp.TX_NOKEY] == 1 and tx.state[1, srtp.TX_PROTECTED] == 1
    assert rx.push(1, prot) is None and rx.state[1, srtp.RX_NOKEY] == 1 and rx.state[1, srtp.RX_OK] == 0
    # held, stopped and silent rows move nothing
    before = tx.state.copy()
    out = tx.protect(packets, [0, 0])
    assert not out["nbytes"].any() and not out["packets"].any() and np.array_equal(tx.state, before)


def test_records_form_equals_the_pushes():
    tx, rx = _pair(3)
    twin = _pair(3)[1]
    arrived, want = [], []
    for seq in range(3):
        for slot in (2, 0):
            plain, prot = _send(tx, slot, seq, bytes([slot, seq]))
            arrived.append((slot, prot))
    arrived.append((0, arrived[1][1]))                       # a duplicate
    fresh = _send(tx, 2, 3)[1]
    arrived.append((2, fresh[:-1] + bytes([fresh[-1] ^ 1])))  # a forgery of a packet not seen yet
    slots = [s for s, _ in arrived]
    rows = np.zeros((len(arrived), TB + 10), dtype=np.uint8)
    for a, (_, p) in enumerate(arrived):
        rows[a, :len(p)] = np.frombuffer(p, dtype=np.uint8)
    rec, offs = forward.arrival_records(slots, rows, [len(p) for _, p in arrived], TB + 10, 3, 12)
    plain = rx.unprotect(rec, offs)
    assert plain.shape == (12, 1 + (TB + 3) // 4)
    order = np.argsort(np.asarray(slots), kind="stable")
    for a, src in enumerate(order):
        got = twin.push(slots[src], arrived[src][1])
        assert plain[a, 0] == (0 if got is None else len(got))
        assert plain[a].view(np.uint8)[4:4 + TB].tobytes() == (got or b"").ljust(TB, b"\0")
    assert np.array_equal(rx.state, twin.state) and not plain[len(arrived):].any()
    assert rx.state[:, srtp.RX_OK].tolist() == [3, 0, 3] and rx.state[0, srtp.RX_REPLAY] == 1 and rx.state[2, srtp.RX_AUTH_FAIL] == 1


# ---------------------------------------------------------------- keys
def test_key_rules_and_value_errors():
    keys = srtp.KeyTable(2)
    k, s = bytes(range(16)), bytes(range(14))
    with pytest.raises(ValueError):
        keys.started(0)                                      # a start without a key
    keys.set_key(0, k, s)
    assert keys.rows[0, srtp.KEY_SSRC] == 0 and keys.dirty
    keys.started(0)
    with pytest.raises(ValueError):
        keys.started(0)                                      # the same key for a second start: SEQ restarts at 0
    with pytest.raises(ValueError):
        keys.set_key(0, k, s)                                # equal to the slot's previous one
    keys.set_key(0, k, s, ssrc=7)                            # another SSRC is another keystream
    keys.set_key(1, k, s)                                    # ... and so is another slot's default SSRC
    keys.started(0)
    for bad in ((k[:15], s), (k + b"\0", s), (k, s[:13]), (k, s + b"\0"), ("0" * 16, s), (k, None), (5, s)):
        with pytest.raises(ValueError) as err:
            keys.set_key(1, *bad)
        assert k.hex() not in str(err.value) and repr(k) not in str(err.value)
    for kw in (dict(ssrc=-1), dict(ssrc=1 << 32), dict(ssrc=True), dict(roc=-1), dict(roc=1 << 32), dict(roc=1.5)):
        with pytest.raises(ValueError):
            keys.set_key(1, bytes(16), s, **kw)
    for slot in (-1, 2, True, 0.0):
        with pytest.raises(ValueError):
            keys.set_key(slot, k, s)
    keys.clear_key(0)
    assert not keys.rows[0].any()
    assert k.hex() not in repr(keys) and "keyed=1" in repr(keys)
    keys.reset()
    assert not keys.rows.any() and keys.last == [None, None]
    with pytest.raises(ValueError):
        srtp.SrtpConfig(profile="AES_256_GCM")
    assert srtp.SrtpConfig().profile == "AES_CM_128_HMAC_SHA1_80"
    for bad in (3, 1 << 16):
        with pytest.raises(ValueError):
            srtp.SenderModel(1, bad)
        with pytest.raises(ValueError):
            srtp.ReceiverModel(1, bad)


def test_a_key_a_slot_was_started_under_never_comes_back():
    """set_key(A), start, set_key(B), set_key(A), start would run A's keystream from SEQ 0 a second time: the second set_key(A) is
    refused, with B started in between or not, on that slot only and until a reset"""
    keys = srtp.KeyTable(2)
    a, b, c, s = bytes(range(16)), bytes(range(1, 17)), bytes(range(2, 18)), bytes(range(14))
    keys.set_key(0, a, s)
    keys.started(0)
    keys.set_key(0, b, s)
    with pytest.raises(ValueError):
        keys.set_key(0, a, s)                                # B was never started: A is still the last key started
    assert np.array_equal(keys.rows[0], srtp.key_row(b, s, 0)) and keys.fresh[0]
    keys.started(0)
    keys.set_key(0, c, s)
    for old in (a, b):
        with pytest.raises(ValueError):
            keys.set_key(0, old, s)
    keys.set_key(1, a, s)                                    # another slot (its SSRC is 1) keeps its own record
    keys.set_key(0, b, s, ssrc=9)                            # and another SSRC is another keystream
    keys.reset()
    keys.set_key(0, a, s)
