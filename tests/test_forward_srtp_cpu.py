"""CPU: SRTP on the forwarding hop (hilcodec_amd/forward_srtp.py, the definition of hilc_srtp_protect_routes and of
GraphedForwardHop(srtp=)): the route row against the C header, RouteModel on scripted traces (every restart cause, the wrap, a late
packet from before it, duplicates, the window's edge, v = -1, no key, epoch saturation), senders -> ForwarderModel -> clients end to
end against the plain forwarder, and the property the epochs exist for: no (key, SSRC, index) is ever encrypted twice.  Everything is
integer: every comparison is exact."""
import re

import numpy as np
import pytest
import torch

from hilcodec_amd import downlink, forward, forward_srtp, rate, srtp, wire
from hilcodec_amd.forward_srtp import (MAX_EPOCH, RT_EPOCH, RT_EXHAUSTED, RT_NOKEY, RT_PROTECTED, RT_ROC, RT_SEEN, RT_SL, RT_STALE, RT_WIN_HI,
                                       RT_WIN_LO, RT_WORDS, ForwarderModel, RouteModel, route_ssrc)
from tests.forward_loop import Membership
from tests.forward_srtp_loop import Call, Clients, forge, key
from tests.hops import HEADER, arrival_arrays, assert_entry_points

TB = 20


# ---------------------------------------------------------------- layout and entry point
def test_layout_matches_header():
    """forward_srtp.<NAME> is `#define HILC_FSRTP_<NAME>`, value for value, in both directions; the row is dense and RT_NAMES are its
    counters"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    env, header = {}, {}
    for name, expr in re.findall(r"^#define (HILC_\w+)[ \t]+(\S.*?)[ \t]*$", text, re.M):
        env[name] = eval(re.sub(r"\b(0x[0-9A-Fa-f]+|\d+)[uU]\b", r"\1", expr), {"__builtins__": {}}, env)
        if name.startswith("HILC_FSRTP_"):
            header[name[len("HILC_FSRTP_"):]] = env[name]
    python = {k: v for k, v in vars(forward_srtp).items() if k.isupper() and isinstance(v, int) and not isinstance(v, bool)}
    assert len(header) == 13 and header == python
    assert sorted(v for k, v in header.items() if k.startswith("RT_") and k != "RT_WORDS") == list(range(RT_WORDS))
    assert [getattr(forward_srtp, "RT_" + n.upper()) for n in forward_srtp.RT_NAMES] == list(range(RT_PROTECTED, RT_WORDS))
    assert MAX_EPOCH == (1 << 28) - 1 and forward.MAX_FANOUT * MAX_EPOCH + forward.MAX_FANOUT - 1 < 1 << 32
    # a key's routes never share an SSRC: (route, epoch) -> SSRC is one to one
    assert len({route_ssrc(5, j, e) for j in range(forward.MAX_FANOUT) for e in (0, 1, 2, MAX_EPOCH)}) == 4 * forward.MAX_FANOUT
    assert route_ssrc(0xFFFFFFFF, 3, 2) == (0xFFFFFFFF + 16 + 3) & 0xFFFFFFFF


def test_entry_point_is_declared_exported_and_bound():
    assert_entry_points(("hilc_srtp_protect_routes",), in_abi16_line=True)
    import hilcodec_amd
    assert callable(hilcodec_amd.srtp_protect_routes) and hilcodec_amd.forward_srtp is forward_srtp


# ---------------------------------------------------------------- RouteModel on scripted traces
def _pkt(seq, fill=0x5A, size=9):
    return bytes([seq >> 8, seq & 255, 0x01]) + bytes([fill]) * (size - 3)


class _Script:
    """a RouteModel of 3 listeners with 2 routes of 2 rows; listener 2 has no key"""

    def __init__(self):
        self.B, self.F, self.P = 3, 2, 2
        self.model = RouteModel(self.B, self.F, self.P, TB)
        for b in (0, 1):
            self.model.keys.set_key(b, *key(9, b), ssrc=100 * b + 5)
        self.model.sent = []
        self.routes = np.array([[1, 2], [0, 2], [0, 1]], dtype=np.int32)

    def hop(self, rows=(), new=(), **flags):
        """rows: {(b, j): [packets]}; new: the (b, j) with new_routes; flags: action / rekey_up / rekey_down = [slots]"""
        B, F, P = self.B, self.F, self.P
        data, nbytes = np.zeros((B, F, P, TB), dtype=np.uint8), np.zeros((B, F, P), dtype=np.int32)
        for (b, j), packets in dict(rows).items():
            for k, p in enumerate(packets):
                data[b, j, k, :len(p)], nbytes[b, j, k] = np.frombuffer(p, dtype=np.uint8), len(p)
        new_routes = np.zeros((B, F), dtype=np.int32)
        for b, j in new:
            new_routes[b, j] = 1
        marks = {}
        for name in ("action", "rekey_up", "rekey_down"):
            marks[name] = np.zeros(B, dtype=np.int32)
            marks[name][list(flags.get(name, ()))] = 1
        res = self.model.protect(data, nbytes, self.routes, new_routes, **marks)
        assert not (res["out"].reshape(-1, TB + 10)[np.arange(B * F * P), :][res["out_nbytes"].reshape(-1) == 0]).any()
        return res

    def want(self, b, j, p, roc):
        """what listener b's client must see on route j for packet p under rollover counter roc"""
        row = self.model.keys.rows[b].copy()
        row[srtp.KEY_SSRC] = srtp._i32(route_ssrc(100 * b + 5, j, int(self.model.state[b, j, RT_EPOCH])))
        return srtp.protect_packet(row, p, roc)


def _row(res, b, j, k):
    return res["out"][b, j, k, :res["out_nbytes"][b, j, k]].tobytes()


def test_each_restart_cause_bumps_the_epoch_of_the_routes_it_touches():
    s = _Script()
    st = s.model.state
    s.hop({(0, 0): [_pkt(7)], (0, 1): [_pkt(7)], (1, 0): [_pkt(7)], (1, 1): [_pkt(7)]})
    assert not st[:, :, RT_EPOCH].any() and st[:2, :, RT_SEEN].all() and (st[:2, :, RT_SL] == 7).all()
    want = np.zeros((3, 2), dtype=np.int64)
    for flags, new, touched in ((dict(), [(0, 0)], [(0, 0)]),                          # new_routes[b][j]
                                (dict(action=[0]), [], [(0, 0), (0, 1), (1, 0), (2, 0)]),  # the listener, and the routes it owns
                                (dict(rekey_down=[1]), [], [(1, 0), (1, 1)]),
                                (dict(action=[2]), [], [(2, 0), (2, 1), (0, 1), (1, 1)]),  # action[t]
                                (dict(rekey_up=[1]), [], [(0, 0), (2, 1)])):               # rekey_up[t]
        st[:2, :, RT_SL], st[:2, :, RT_SEEN], st[:2, :, RT_ROC], st[:2, :, RT_WIN_LO] = 7, 1, 3, 5
        before = st.copy()
        s.hop(new=new, **flags)
        for b, j in touched:
            want[b, j] += 1
        assert np.array_equal(st[:, :, RT_EPOCH], want), flags
        for b in range(2):
            for j in range(2):
                if (b, j) in touched:
                    assert not st[b, j, RT_ROC:RT_WIN_HI + 1].any(), (flags, b, j)
                else:
                    assert np.array_equal(st[b, j], before[b, j]), (flags, b, j)
        assert np.array_equal(st[:, :, RT_PROTECTED:], before[:, :, RT_PROTECTED:])          # counters survive
    # a route without an owner ignores whoever restarts; a restarted route sends its next packet under its new SSRC from ROC 0
    s.routes[0, 0] = -1
    s.hop(action=[1], rekey_up=[1])
    assert st[0, 0, RT_EPOCH] == want[0, 0]
    s.routes[0, 0] = 1
    res = s.hop({(0, 0): [_pkt(7)]})
    assert _row(res, 0, 0, 0) == s.want(0, 0, _pkt(7), 0) and st[0, 0, RT_EPOCH] == 3
    assert len(set(s.model.sent)) == len(s.model.sent) == 5


def test_wrap_late_duplicate_window_edge_v_minus_one_nokey_and_saturation():
    s = _Script()
    st = s.model.state
    seen = np.zeros(RT_WORDS, dtype=np.int64)
    # a SEQ run across 0xFFFF gives ROC 1, two rows per hop
    res = s.hop({(0, 0): [_pkt(0xFFFE), _pkt(0xFFFF)]})
    assert [_row(res, 0, 0, k) for k in (0, 1)] == [s.want(0, 0, _pkt(0xFFFE), 0), s.want(0, 0, _pkt(0xFFFF), 0)]
    res = s.hop({(0, 0): [_pkt(0x0000), _pkt(0x0001)]})
    assert [_row(res, 0, 0, k) for k in (0, 1)] == [s.want(0, 0, _pkt(0), 1), s.want(0, 0, _pkt(1), 1)]
    assert st[0, 0, RT_ROC] == 1 and st[0, 0, RT_SL] == 1 and st[0, 0, RT_WIN_LO] == 0b1111 and st[0, 0, RT_PROTECTED] == 4
    # a late packet from before the wrap goes out under ROC - 1 and moves neither ROC nor top
    res = s.hop({(0, 0): [_pkt(0xFFFD, 0x33)]})
    assert _row(res, 0, 0, 0) == s.want(0, 0, _pkt(0xFFFD, 0x33), 0)
    assert st[0, 0, RT_ROC] == 1 and st[0, 0, RT_SL] == 1 and st[0, 0, RT_WIN_LO] == 0b11111
    # a duplicate — of the top, of the late one, with another body — is refused: zero row, count 0, the row unchanged
    before = st[0, 0].copy()
    res = s.hop({(0, 0): [_pkt(0x0001), _pkt(0xFFFD, 0x77)]})
    assert not res["out_nbytes"].any() and not res["out"].any()
    before[RT_STALE] += 2
    assert np.array_equal(st[0, 0], before)
    # the window's edge: 63 below the top goes, 64 below does not
    s.hop({(0, 0): [_pkt(0x0050)]})
    res = s.hop({(0, 0): [_pkt(0x0010), _pkt(0x0011)]})
    assert res["out_nbytes"][0, 0].tolist() == [0, len(_pkt(0)) + 10] and _row(res, 0, 0, 1) == s.want(0, 0, _pkt(0x11), 1)
    assert st[0, 0, RT_STALE] == 3 and st[0, 0, RT_WIN_HI] == -0x80000000
    # a first packet, then an older one from before the wrap: v = -1 at ROC 0, refused
    res = s.hop({(1, 1): [_pkt(0x0002), _pkt(0xFFF0)]})
    assert res["out_nbytes"][1, 1].tolist() == [len(_pkt(0)) + 10, 0] and st[1, 1, RT_STALE] == 1 and st[1, 1, RT_ROC] == 0
    # no key: nothing leaves, whatever the route
    res = s.hop({(2, 0): [_pkt(1), _pkt(2)], (2, 1): [_pkt(1)]})
    assert not res["out"].any() and st[2, :, RT_NOKEY].tolist() == [2, 1] and not st[2, :, :RT_NOKEY].any()
    # a row below the header is nothing at all
    before = st.copy()
    res = s.hop({(0, 0): [b"\x00\x60"], (2, 0): [b"\x01"]})
    assert not res["out"].any() and np.array_equal(st, before)
    seen += np.abs(st).sum(axis=(0, 1))
    # epoch saturation, preset: the last epoch still sends, a restart there ends the route for good
    st[1, 0, RT_EPOCH] = MAX_EPOCH - 1
    res = s.hop({(1, 0): [_pkt(3)]}, new=[(1, 0)])
    assert st[1, 0, RT_EPOCH] == MAX_EPOCH and _row(res, 1, 0, 0) == s.want(1, 0, _pkt(3), 0)
    for flags in (dict(rekey_up=[0]), dict(), dict(action=[1])):
        res = s.hop({(1, 0): [_pkt(4), _pkt(5)]}, **flags)
        assert not res["out"].any() and st[1, 0, RT_EPOCH] == MAX_EPOCH and st[1, 0, RT_SEEN] == forward_srtp.SEEN_EXHAUSTED
    assert st[1, 0, RT_EXHAUSTED] == 6 and st[1, 0, RT_PROTECTED] == 1
    seen += np.abs(st).sum(axis=(0, 1))
    assert all(seen[getattr(forward_srtp, "RT_" + name.upper())] > 0 for name in forward_srtp.RT_NAMES)
    assert len(set(s.model.sent)) == len(s.model.sent)


# ---------------------------------------------------------------- end to end on the host
B, N, T, M, K = 6, 4, 1, 1, 4
CFG = forward.ForwardConfig(fanout=2, burst=2, hang_hops=3)


def _setup(call, fm, clients, b):
    mk, ms, ssrc = call.rekey(b)
    fm.keys.set_uplink_key(b, mk, ms, ssrc=ssrc)
    dk, ds = key(500, b)
    fm.keys.set_downlink_key(b, dk, ds, ssrc=77 * b)
    clients.set_key(b, dk, ds, 77 * b)


@pytest.mark.parametrize("rated", [False, True], ids=["plain", "rate"])
def test_senders_forwarder_clients_end_to_end(rated):
    """36 hops of 6 slots in 2 rooms: every row a client decrypts is the row the plain forwarder (with `rated`: behind its downlink
    rate model) makes from the plaintext; a forged arrival counts RX_AUTH_FAIL and SD_MALFORMED and reaches nobody"""
    dl = downlink.DownlinkConfig(rate=rate.RateConfig(min_kbps=9.0, max_kbps=24.0)) if rated else None
    tb = wire.transport_bytes(N, M, T)
    call = Call(B, N, T, M, K, seed=5, first={1: 0xFFF6}, late=(2, 4))
    fm = ForwarderModel(B, CFG, N, T, M, K, downlink=dl)
    ref = downlink.ForwardDownlinkModel(B, CFG, dl, N, T, M, K) if rated else forward.ForwardModel(B, CFG, N, T, M, K)
    clients = Clients(B, CFG.fanout, tb)
    members = Membership(B, N)
    members.apply([("join", b, b % 2) for b in range(B)])
    for b in range(B):
        _setup(call, fm, clients, b)
    forged, wrapped = 0, False
    for h in range(36):
        if h == 12:
            members.apply([("join", 3, 0), ("layers", 0, 2)])
        if h == 20:                                          # sender 5 starts again under a new key, listener 2 gets a new downlink key
            mk, ms, ssrc = call.rekey(5)
            fm.keys.set_uplink_key(5, mk, ms, ssrc=ssrc)
            dk, ds = key(501, 2)
            fm.keys.set_downlink_key(2, dk, ds, ssrc=9)
            clients.set_key(2, dk, ds, 9)
        plain, wired = call.hop()
        if h == 15 and wired:
            wired = [(wired[0][0], forge(wired[0][1]))] + wired
            forged = wired[0][0]
        action = members.action()
        reports = ([0, 3], [0, 1], [wire.pack_report(h & 255, 40 if h > 18 else 0, 0)] * 2) if rated and h % 5 == 4 else None
        got = fm.step(*arrival_arrays(wired, tb + 10), members.room, members.layers, action, reports=reports)
        extra = dict(reports=reports) if rated else {}
        want = ref.step(*arrival_arrays(plain, tb), members.room, members.layers, action, **extra)
        rows, counts = clients.deliver(fm.egress.state[:, :, RT_EPOCH], got["out"], got["out_nbytes"])
        assert np.array_equal(counts, want["out_nbytes"]), h
        assert np.array_equal(rows, want["out"]), h
        assert np.array_equal(got["out_nbytes"], np.where(want["out_nbytes"] > 0, want["out_nbytes"] + 10, 0)), h
        assert np.array_equal(got["routes"], want["routes"]) and np.array_equal(got["new_routes"], want["new_routes"]), h
        wrapped = wrapped or bool((fm.egress.state[:, :, RT_ROC] == 1).any())
    sd, sd_ref = fm.sender.state, (ref.forward if rated else ref).sender.state.copy()
    sd_ref[forged, forward.SD_MALFORMED] += 1
    assert np.array_equal(sd, sd_ref)
    assert fm.ingress.state[:, srtp.RX_AUTH_FAIL].sum() == 1 and fm.ingress.state[forged, srtp.RX_AUTH_FAIL] == 1
    assert np.array_equal(fm.listener.state, (ref.forward if rated else ref).listener.state)
    if rated:
        assert np.array_equal(fm.downlink.state, ref.downlink.state)
    assert clients.delivered > 100 and fm.egress.state[:, :, RT_PROTECTED].sum() == clients.delivered
    assert fm.ingress.state[1, srtp.RX_ROC] == 1 and wrapped                    # the wrap went through both sides
    assert fm.egress.state[2, :, RT_EPOCH].min() >= 2 and not fm.egress.state[:, :, RT_NOKEY:].any()


def test_no_key_ssrc_index_is_ever_used_twice():
    """400 hops of 6 slots in 2 rooms, fanout 2, burst 2, with sender restarts under new keys, re-joins, reordered and duplicated
    arrivals and downlink re-keys: the (downlink key, SSRC, index) of every protected row is distinct, and not because everything
    was dropped — the egress refuses at most 1 forwarded row in 10 (this seed: 3 431 rows protected under 18 keys and 465 SSRCs, none
    refused at the egress, since the ingress has already rejected the 56 repeats; the test below feeds the egress directly)"""
    tb = wire.transport_bytes(N, M, T)
    call = Call(B, N, T, M, None, seed=23, first={0: 0xFF40, 3: 0xFFC0}, late=(1, 2, 3))
    fm = ForwarderModel(B, CFG, N, T, M, None)
    fm.egress.sent = []
    clients = Clients(B, CFG.fanout, tb)                     # key book-keeping only: nothing is decrypted here
    members = Membership(B, N)
    members.apply([("join", b, b % 2) for b in range(B)])
    for b in range(B):
        _setup(call, fm, clients, b)
    rng = np.random.default_rng(99)
    down_gen = 600
    for h in range(400):
        what = rng.random()
        b = int(rng.integers(0, B))
        if what < 0.04:
            mk, ms, ssrc = call.rekey(b)
            fm.keys.set_uplink_key(b, mk, ms, ssrc=ssrc)
        elif what < 0.08:
            members.apply([("join", b, int(rng.integers(0, 2)))])
        elif what < 0.11:
            down_gen += 1
            fm.keys.set_downlink_key(b, *key(down_gen, b), ssrc=77 * b)      # a new key under the same base SSRC
        plain, wired = call.hop(p_flip=0.2)
        if h > 2 and rng.random() < 0.3:                     # an arrival of an earlier hop once more
            old = call.history[int(rng.integers(max(0, h - 6), h))]
            if old:
                wired.append(old[int(rng.integers(0, len(old)))])
        fm.step(*arrival_arrays(wired, tb + 10), members.room, members.layers, members.action())
    sent, st = fm.egress.sent, fm.egress.state
    assert len(sent) == st[:, :, RT_PROTECTED].sum() > 2000
    assert len(set(sent)) == len(sent)
    assert len({s[0] for s in sent}) > B and len({s[1] for s in sent}) > 40 and max(s[2] for s in sent) >> 16 == 1
    assert 10 * st[:, :, RT_STALE].sum() <= st[:, :, RT_PROTECTED].sum() + st[:, :, RT_STALE].sum()
    assert fm.ingress.state[:, srtp.RX_REPLAY].sum() > 20 and fm.ingress.state[:, srtp.RX_AUTH_FAIL].sum() > 0
    assert st[:, :, RT_EPOCH].min() >= 2 and not st[:, :, RT_NOKEY].any()


def test_the_egress_alone_never_reuses_an_index_whatever_it_is_fed():
    """in the trace above the ingress rejects every repeat, so the egress refuses nothing (RT_STALE stays 0 there).  Here RouteModel is
    fed directly, as by an ingress that lets everything through: one row in three repeats a SEQ of the last few rows or comes late,
    SEQs cross the wrap, owners and flags change at random.  Still no (key, SSRC, index) twice; what it refuses is counted"""
    Bn, F, P = 4, 3, 4
    model = RouteModel(Bn, F, P, TB)
    for b in range(Bn):
        model.keys.set_key(b, *key(40, b), ssrc=b)           # bases 0..3 with 3 routes each: the routes' SSRCs interleave
    model.sent = []
    rng = np.random.default_rng(8)
    nxt = np.full((Bn, F), 0xFFF0, dtype=np.int64)
    for h in range(60):
        rows, nbytes = np.zeros((Bn, F, P, TB), dtype=np.uint8), np.zeros((Bn, F, P), dtype=np.int32)
        for b, j, k in np.ndindex(Bn, F, P):
            if rng.random() < 0.2:
                continue
            seq = int(nxt[b, j])
            if rng.random() < 0.33:
                seq = (seq - int(rng.integers(1, 70))) & 0xFFFF
            else:
                nxt[b, j] = (nxt[b, j] + 1) & 0xFFFF
            p = _pkt(seq, int(rng.integers(0, 256)), int(rng.integers(4, TB + 1)))
            rows[b, j, k, :len(p)], nbytes[b, j, k] = np.frombuffer(p, dtype=np.uint8), len(p)
        flags = [(rng.random(Bn) < 0.03).astype(np.int32) for _ in range(3)]
        model.protect(rows, nbytes, rng.integers(-1, Bn, (Bn, F)), (rng.random((Bn, F)) < 0.05).astype(np.int32), *flags)
    st = model.state
    assert len(model.sent) == st[:, :, RT_PROTECTED].sum() and len(set(model.sent)) == len(model.sent)
    assert st[:, :, RT_PROTECTED].sum() > st[:, :, RT_STALE].sum() > 100 and st[:, :, RT_EPOCH].max() > 3
    assert max(s[2] for s in model.sent) >> 16 == 1


# ---------------------------------------------------------------- errors
def test_constructor_and_key_errors():
    from hilcodec_amd.graph_step import GraphedForwardHop
    nack = downlink.DownlinkConfig(history=8)
    with pytest.raises(ValueError, match="history"):
        ForwarderModel(B, CFG, N, T, M, K, downlink=nack)
    with pytest.raises(ValueError, match="history"):         # refused before anything touches a device
        GraphedForwardHop(B, T, N, torch.device("cpu"), fec_stages=M, cfg=CFG, downlink=nack, srtp=srtp.SrtpConfig())
    with pytest.raises(ValueError):
        GraphedForwardHop(B, T, N, torch.device("cpu"), cfg=CFG, srtp="AES_CM_128_HMAC_SHA1_80")
    keys = forward_srtp.ForwardKeys(3)
    secret = bytes(range(0xA0, 0xAF))
    for call in (lambda: keys.set_uplink_key(0, secret, bytes(14)), lambda: keys.set_downlink_key(0, bytes(16), secret + b"\x01\x02"),
                 lambda: keys.set_uplink_key(0, secret.hex(), bytes(14))):
        with pytest.raises(ValueError) as err:
            call()
        assert secret.hex() not in str(err.value).lower() and repr(secret) not in str(err.value) and "a0a1" not in str(err.value)
    with pytest.raises(ValueError):
        keys.set_downlink_key(3, bytes(16), bytes(14))
    with pytest.raises(ValueError):
        keys.set_uplink_key(0, bytes(16), bytes(14), roc=-1)
    assert not keys.pending
    keys.set_uplink_key(1, bytes(16), bytes(14))
    keys.set_downlink_key(2, bytes(16), bytes(14))
    with pytest.raises(ValueError):
        keys.set_uplink_key(1, bytes(16), bytes(14))         # the key it had before
    assert keys.pending and keys.take() == ([1], [2]) and not keys.pending and keys.take() == ([], [])
    assert "00" * 8 not in repr(keys)
    with pytest.raises(ValueError):
        RouteModel(2, 9, 2, TB)
    with pytest.raises(ValueError):
        RouteModel(2, 2, 2, 3)
