"""GPU: SRTP packet protection of the graphed hops (GraphedEncodeHop(srtp=SrtpConfig()), GraphedDecodeHop(srtp=SrtpConfig())).
hilc_srtp_protect and hilc_srtp_unprotect against srtp.py's models word for word — every AES block edge and SHA-1 padding edge, slots
without a key, starts, the rollover, duplicates and forgeries, aligned rows and 4-byte-skewed views — then the protecting sender
against the plain sender and the protected receiver against the plain receiver.  Every comparison is bit for bit."""
import numpy as np
import pytest
import torch

from hilcodec_amd import forward, srtp, wire
from tests.alignment import skew
from tests.hops import SRTP_LENGTHS as LENGTHS

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
B_KERNEL = 67                                                # two workgroups of 64, the second a partial wave
TB = 80
UNKEYED = (5, 64)


def dev(a, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).to(DEV)


def _keyed(model, seed):
    rng = np.random.default_rng(seed)
    for b in range(model.B):
        if b not in UNKEYED:
            model.keys.set_key(b, rng.integers(0, 256, 16, dtype=np.uint8).tobytes(), rng.integers(0, 256, 14, dtype=np.uint8).tobytes(),
                               ssrc=int(rng.integers(0, 1 << 32)), roc=int(b % 3 == 0) * 0x01020304)
    return rng


def _traffic(rng, seq, tb, row_bytes=None):
    """one hop of headed rows: every length of LENGTHS over the slots, garbage past the byte count"""
    B = len(seq)
    packets = rng.integers(0, 256, (B, row_bytes or tb), dtype=np.uint8)
    nbytes = np.array([LENGTHS[int(i)] for i in rng.integers(0, len(LENGTHS), B)], dtype=np.int32)
    nbytes = np.minimum(nbytes, tb)
    packets[:, 0], packets[:, 1] = seq >> 8, seq & 255
    return packets, nbytes


@pytest.mark.parametrize("tb, views", [(TB, False), (TB, True), (41, False), (41, True), (78, False)],
                         ids=["aligned", "aligned-skewed", "odd", "odd-skewed", "out-aligned"])
def test_protect_kernel(tb, views):
    """hops of every length on 67 slots against SenderModel: rows, byte counts and TX rows; slots without a key, starts with a ROC
    from the key row, rows pre-set to 0xFFFE so that the run crosses the wrap.  `views`: every tensor 4, 8 or 12 bytes off a
    16-byte boundary — an aligned width (80) then takes the word path from a skewed base, an odd one (41) the byte path"""
    from hilcodec_amd import ops
    B = B_KERNEL
    model = srtp.SenderModel(B, tb)
    rng = _keyed(model, 11 + tb)
    keys = dev(model.keys.rows)
    model.protect(np.zeros((B, tb), dtype=np.uint8), np.zeros(B, dtype=np.int32), np.ones(B, dtype=np.int32))     # the keys' ROCs
    model.state[:, srtp.TX_LAST], model.state[:, srtp.TX_SENT] = 0xFFFE, 1
    model.state[7, srtp.TX_ROC] = -1                         # 2^32 - 1: the counter wraps, too
    rows = dev(model.state)
    seq = np.full(B, 0xFFFE, dtype=np.int64)
    out = torch.full((B, tb + 10), 0xAB, dtype=torch.uint8, device=DEV)
    out_nb = torch.full((B,), -9, dtype=torch.int32, device=DEV)
    seen = set()
    for k in range(8):
        packets, nbytes = _traffic(rng, seq, tb)
        action = (rng.random(B) < 0.1).astype(np.int32) * (k > 0) * rng.choice([-1, 1, 3], B).astype(np.int32)
        want = model.protect(packets, nbytes, action)
        args = [dev(packets, np.uint8), dev(nbytes), keys, rows, out, out_nb, dev(action)]
        if views:
            args = [skew(t, 1 + (i + k) % 3) for i, t in enumerate(args)]
        ops.srtp_protect(*args[:4], out=args[4], out_nbytes=args[5], action=args[6])
        if views:
            rows.copy_(args[3])
        assert np.array_equal(args[5].cpu().numpy(), want["nbytes"]), k
        assert np.array_equal(args[4].cpu().numpy(), want["packets"]), k
        assert np.array_equal(rows.cpu().numpy(), model.state), k
        assert np.array_equal(args[0].cpu().numpy(), packets)                    # read only
        seen |= set(nbytes[[b for b in range(B) if b not in UNKEYED]].tolist())
        seq = (seq + (nbytes >= 3)) & 0xFFFF
    st = model.state
    assert seen == set(min(v, tb) for v in LENGTHS)
    assert st[list(UNKEYED), srtp.TX_NOKEY].min() >= 1 and not st[list(UNKEYED), srtp.TX_PROTECTED].any()
    assert (st[:, srtp.TX_ROC] == 1).any() and (st[:, srtp.TX_ROC] == 0x01020305).any()
    # without an action row no slot is cleared
    packets, nbytes = _traffic(rng, seq, tb)
    want = model.protect(packets, nbytes)
    got, got_nb = ops.srtp_protect(dev(packets, np.uint8), dev(nbytes), keys, rows)
    assert np.array_equal(got.cpu().numpy(), want["packets"]) and np.array_equal(got_nb.cpu().numpy(), want["nbytes"])
    assert np.array_equal(rows.cpu().numpy(), model.state)


@pytest.mark.parametrize("tb, views", [(TB, False), (TB, True), (41, False)], ids=["aligned", "skewed", "odd"])
def test_unprotect_kernel(tb, views):
    """several arrivals per slot and hop — genuine ones of every length in shuffled order, duplicates, forgeries (a flipped bit in
    the header, the body or the tag), truncations, byte counts past the record — against ReceiverModel: records, RX rows"""
    from hilcodec_amd import ops
    B, max_a = B_KERNEL, 4 * B_KERNEL
    tx, model = srtp.SenderModel(B, tb), srtp.ReceiverModel(B, tb)
    _keyed(tx, 3)
    rng = _keyed(model, 3)
    keys = dev(model.keys.rows)
    start = np.ones(B, dtype=np.int32)
    tx.protect(np.zeros((B, tb), dtype=np.uint8), np.zeros(B, dtype=np.int32), start)
    tx.state[:, srtp.TX_LAST], tx.state[:, srtp.TX_SENT] = 0xFFFE, 1
    model.start(start)
    model.state[::2, srtp.RX_SL], model.state[::2, srtp.RX_SEEN] = 0xFFFE, 1
    model.state[::2, srtp.RX_WIN_LO], model.state[::2, srtp.RX_WIN_HI] = -0x7FFFFFFF, 0x40000000      # bits that cross the two words
    rows = dev(model.state)
    seq = np.full(B, 0xFFFF, dtype=np.int64)
    plain = torch.full((max_a, 1 + (tb + 3) // 4), -7, dtype=torch.int32, device=DEV)
    history = []
    for k in range(8):
        arrived = []
        for _ in range(2):
            packets, nbytes = _traffic(rng, seq, tb)
            out = tx.protect(packets, nbytes)
            seq = (seq + (nbytes >= 3)) & 0xFFFF
            for b in np.nonzero(out["nbytes"])[0]:
                arrived.append((int(b), out["packets"][b, :out["nbytes"][b]].tobytes()))
        history += arrived
        for _ in range(12):
            b, p = history[int(rng.integers(0, len(history)))]
            kind = int(rng.integers(0, 4))
            if kind == 0:
                arrived.append((b, p))                                            # a duplicate, or a packet far in the past
            elif kind == 1:
                bit = int(rng.integers(0, 8 * len(p)))
                arrived.append((b, p[:bit >> 3] + bytes([p[bit >> 3] ^ (1 << (bit & 7))]) + p[(bit >> 3) + 1:]))
            elif kind == 2:
                arrived.append((b, p[:int(rng.integers(0, len(p)))]))
            else:
                arrived.append((int(rng.integers(0, B)), p))                      # another slot's packet
        arrived += [(u, history[0][1]) for u in UNKEYED]
        arrived = [arrived[i] for i in rng.permutation(len(arrived))]
        assert len(arrived) <= max_a
        slots = [s for s, _ in arrived]
        data = np.zeros((len(arrived), tb + 10), dtype=np.uint8)
        for a, (_, p) in enumerate(arrived):
            data[a, :len(p)] = np.frombuffer(p, dtype=np.uint8)
        counts = [len(p) for _, p in arrived]
        counts[0], counts[1] = tb + 11, -1                                        # a count past the record, a negative one
        rec, offs = forward.arrival_records(slots, data, counts, tb + 10, B, max_a)
        action = (rng.random(B) < 0.05).astype(np.int32) * (k > 0)
        want = model.unprotect(rec, offs, action)
        args = [dev(rec), dev(offs), keys, rows, plain, dev(action)]
        if views:
            args = [skew(t, 1 + (i + k) % 3) for i, t in enumerate(args)]
        plain.fill_(-7)
        if views:
            args[4].fill_(-7)
        ops.srtp_unprotect(*args[:4], tb, plain=args[4], action=args[5])
        if views:
            rows.copy_(args[3])
        got = args[4].cpu().numpy()
        assert np.array_equal(got[:len(arrived)], want[:len(arrived)]), k
        assert (got[len(arrived):] == -7).all()                                   # outside every slot's range: not written
        assert np.array_equal(rows.cpu().numpy(), model.state), k
        assert np.array_equal(args[0].cpu().numpy(), rec)                         # read only
    st = model.state
    keyed = [b for b in range(B) if b not in UNKEYED]
    assert all(st[keyed, i].sum() > 0 for i in range(srtp.RX_OK, srtp.RX_NOKEY)), st[:, srtp.RX_OK:].sum(axis=0)
    assert st[list(UNKEYED), srtp.RX_NOKEY].min() >= 1 and not st[list(UNKEYED), srtp.RX_OK].any()
    assert (st[:, srtp.RX_ROC] == 1).any() and (st[:, srtp.RX_ROC] == 0x01020305).any()


def test_round_trip_on_the_device_and_known_answer():
    """the RFC 3711 B.3 session keys through both launches: the issue's three whole packets, then back"""
    import hilcodec_amd
    h = bytes.fromhex
    ke, ka, ks = srtp.derive(h("E1F97A0D3E018BE0D64FA32C06DE4139"), h("0EC675AD498AFEEBB6960B3AABE6"))
    cases = [(0xCAFEBABE, 0, 0x1234, 0x08, bytes(range(10)), "123408e5ff75e44837d5742f06a9d11d30e4b1954c8eca"),
             (0xCAFEBABE, 1, 0x0001, 0x48, bytes(range(0x10, 0x1D)), "0001480d4b491ce71c85108e9de41cd21bf93e9df9d65357f277"),
             (0, 0, 0, 0x80, bytes(range(1, 40)),
              "000080fb61bf426d6e5c6df1f017ef9d92e5c55ce916e541a034c5fba126cb0ac1dcdbd42cdf43fd318d0a12f828e5055593a357")]
    tb, B = 42, len(cases)
    keys = np.stack([srtp.session_key_row(ke, ka, ks, c[0], c[1]) for c in cases])
    packets, nbytes = np.zeros((B, tb), dtype=np.uint8), np.zeros(B, dtype=np.int32)
    for b, (_, _, seq, flags, body, _) in enumerate(cases):
        blob = bytes([seq >> 8, seq & 255, flags]) + body
        packets[b, :len(blob)], nbytes[b] = np.frombuffer(blob, dtype=np.uint8), len(blob)
    start = dev(np.ones(B))
    tx_rows = torch.zeros(B, srtp.TX_WORDS, dtype=torch.int32, device=DEV)
    out, out_nb = hilcodec_amd.srtp_protect(dev(packets, np.uint8), dev(nbytes), dev(keys), tx_rows, action=start)
    for b, c in enumerate(cases):
        assert bytes(out[b, :int(out_nb[b])].tolist()) == h(c[5]), b
    rec, offs = forward.arrival_records(list(range(B)), out.cpu().numpy(), out_nb.cpu().numpy(), tb + 10, B, B)
    rx_rows = torch.zeros(B, srtp.RX_WORDS, dtype=torch.int32, device=DEV)
    plain = hilcodec_amd.srtp_unprotect(dev(rec), dev(offs), dev(keys), rx_rows, tb, action=start).cpu().numpy()
    want, _ = forward.arrival_records(list(range(B)), packets, nbytes, tb, B, B)
    assert np.array_equal(plain, want) and rx_rows[:, srtp.RX_OK].tolist() == [1, 1, 1]


def test_argument_checks():
    from hilcodec_amd import ops
    B, tb = 3, 20
    ints = dict(dtype=torch.int32, device=DEV)
    pk, nb = torch.zeros(B, tb, dtype=torch.uint8, device=DEV), torch.zeros(B, **ints)
    keys, tx, rx = torch.zeros(B, srtp.KEY_WORDS, **ints), torch.zeros(B, srtp.TX_WORDS, **ints), torch.zeros(B, srtp.RX_WORDS, **ints)
    for bad in (dict(keys=keys[:, :-1].contiguous()), dict(rows=rx), dict(nbytes=nb[:2]), dict(action=nb[:2]),
                dict(out=torch.zeros(B, tb, dtype=torch.uint8, device=DEV)), dict(packets=pk[:, :3].contiguous(), out=None)):
        kw = {**dict(packets=pk, nbytes=nb, keys=keys, rows=tx), **bad}
        with pytest.raises(RuntimeError):
            ops.srtp_protect(**kw)
    rec, offs = torch.zeros(4, 1 + (tb + 13) // 4, **ints), torch.zeros(B + 1, **ints)
    for bad in (dict(keys=keys[:2]), dict(rows=tx), dict(offsets=offs[:3]), dict(arrivals=rec[:, :-1].contiguous()),
                dict(plain=torch.zeros(4, 2, **ints)), dict(row_bytes=3)):
        kw = {**dict(arrivals=rec, offsets=offs, keys=keys, rows=rx, row_bytes=tb), **bad}
        with pytest.raises(RuntimeError):
            ops.srtp_unprotect(**kw)
    with pytest.raises(RuntimeError):
        ops.srtp_protect(pk.cpu(), nb.cpu(), keys.cpu(), tx.cpu())


# ---------------------------------------------------------------- the hops
HOP = 320


@pytest.fixture(scope="module")
def speech():
    from tests.hops import build_streaming
    return build_streaming()[0]


def _key(tag, b):
    return bytes([tag, b] * 8), bytes([b, tag] * 7)


def test_sender_hop_protects_what_the_plain_hop_sends(speech):
    """12 hops at B = 5 with FEC, DTX, a history, rate control, a hold, a slot without a key and a mid-run start under a new key: the
    srtp hop's rows are SenderModel's protect of the plain hop's rows, a NACKed packet comes back byte for byte as it was sent, and
    the rate row differs from the plain hop's only in the credit, by 80 bits per packet sent"""
    from hilcodec_amd import dtx, rate, rtx, synth
    from hilcodec_amd.graph_step import GraphedEncodeHop
    from tests.hops import caches_equal
    B, n, m, hops = 5, 4, 1, 12
    rcfg = rate.RateConfig(4.0, 24.0)
    kw = dict(sessions=True, header=True, fec_stages=m, dtx=dtx.DtxConfig(order=4), rtx=rtx.RtxConfig(8, 2), rate=rcfg)
    tx = GraphedEncodeHop(speech, B, HOP, n, DEV, srtp=srtp.SrtpConfig(), **kw)
    ref = GraphedEncodeHop(speech, B, HOP, n, DEV, **kw)
    tb = wire.transport_bytes(n, m, 1)
    model = srtp.SenderModel(B, tb)
    for b in range(B - 1):                                   # slot 4 has no key
        tx.set_key(b, *_key(1, b), ssrc=7 * b, roc=b % 2)
        model.keys.set_key(b, *_key(1, b), ssrc=7 * b, roc=b % 2)
        tx.start(b)
        ref.start(b)
    bits = rate.bucket(rcfg, 1, m, True)
    r, burst = bits.start_bits, rcfg.burst_hops
    credit = {name: np.full(B, burst * r, dtype=np.int64) for name in ("tx", "ref")}
    x = synth.synth_clips(B, HOP * hops, seed=21).to(DEV)
    x[1, :, HOP * 3:HOP * 10] = 0                            # SIDs and silence on slot 1
    sent = []
    for k in range(hops):
        action = np.zeros(B, dtype=np.int32)
        if k == 0:
            action[:B - 1] = 1
        if k == 6:
            with pytest.raises(ValueError):
                tx.start(2)                                  # no key since its previous start
            tx.set_key(2, *_key(2, 2))
            model.keys.set_key(2, *_key(2, 2))
            tx.start(2)
            ref.start(2)
            action[2] = 1
        holds = [0] if k in (3, 4) else []
        nacks = ([3], [wire.pack_nack(5, 0)]) if k == 8 else None
        xk = x[:, :, HOP * k:HOP * (k + 1)].contiguous()
        (pk, nb), (pk1, nb1) = tx.step(xk, hold=holds, nacks=nacks), ref.step(xk, hold=holds, nacks=nacks)
        assert pk.shape == (B, wire.srtp_bytes(n, m, 1)) and tx.rtx_packets.shape == (B, 2, wire.srtp_bytes(n, m, 1))
        want = model.protect(pk1.cpu().numpy(), nb1.cpu().numpy(), action)
        assert np.array_equal(nb.cpu().numpy(), want["nbytes"]), k
        assert np.array_equal(pk.cpu().numpy(), want["packets"]), k
        assert np.array_equal(tx.srtp_state.cpu().numpy(), model.state), k
        assert torch.equal(tx.indices, ref.indices) and torch.equal(tx.kind, ref.kind) and torch.equal(tx.hop_index, ref.hop_index), k
        assert caches_equal(tx.cache_enc, ref.cache_enc) and torch.equal(tx.n_ceil, ref.n_ceil), k
        sent.append((pk.cpu().clone(), nb.cpu().clone()))
        if k == 8:
            assert int(sent[5][1][3]) > 0 and tx.rtx_nbytes[3].tolist() == [int(sent[5][1][3]), 0]
            assert torch.equal(tx.rtx_packets[3, 0].cpu(), sent[5][0][3])            # ciphertext and tag, as sent
            assert ref.rtx_nbytes[3, 0] == tx.rtx_nbytes[3, 0] - 10
        else:
            assert not tx.rtx_nbytes.any()
        # rate.py's bucket on what each hop put on the wire: the only difference is the 10 bytes behind each sent packet
        for name, hop, count in (("tx", tx, nb), ("ref", ref, nb1)):
            c = credit[name]
            c[action != 0] = burst * r
            free = np.array([b not in holds for b in range(B)])
            c[free] = np.minimum(c[free] + r, burst * r)
            c[:] = np.maximum(c - 8 * (count.cpu().numpy().astype(np.int64) + hop.rtx_nbytes.cpu().numpy().sum(axis=1)), -burst * r)
            assert np.array_equal(hop.rate_state[:, rate.RC_CREDIT].cpu().numpy(), c), (name, k)
        others = [i for i in range(rate.RC_WORDS) if i != rate.RC_CREDIT]
        assert torch.equal(tx.rate_state[:, others], ref.rate_state[:, others]), k
        assert np.array_equal(nb.cpu().numpy(), np.where(want["nbytes"] > 0, nb1.cpu().numpy() + 10, 0)), k
    st = model.state
    assert st[4, srtp.TX_NOKEY] == hops and st[4, srtp.TX_PROTECTED] == 0 and not any(int(s[1][4]) for s in sent)
    assert st[0, srtp.TX_PROTECTED] == hops - 2 and st[2, srtp.TX_PROTECTED] == hops - 6      # held hops send nothing; a start clears
    assert st[1, srtp.TX_PROTECTED] == sum(int(s[1][1]) > 0 for s in sent)                     # SIDs are protected like any packet
    assert st[:4, srtp.TX_ROC].tolist() == [0, 1, 0, 1]
    assert (credit["tx"] < credit["ref"])[[0, 2, 3]].all()
    # keys never show; reset clears rows and keys
    assert _key(1, 0)[0].hex() not in repr(tx._keys) and "keyed=4" in repr(tx._keys)
    with pytest.raises(ValueError):
        tx.set_key(2, *_key(2, 2))                           # the key it had before
    tx.reset()
    assert not tx.srtp_state.any()
    pk, nb = tx.step(xk)
    assert not nb.any() and not pk.any() and tx.srtp_state[:, srtp.TX_NOKEY].tolist() == [1] * B
    tx.set_key(0, *_key(1, 0), ssrc=0, roc=0)                # reset forgot the old keys
    pk, nb = tx.step(xk)
    assert int(nb[0]) > 0 and not nb[1:].any()


def test_receiver_hop_drops_what_does_not_authenticate(speech):
    """the protected rows of a sender plus one forged, one replayed and one truncated arrival on slot 1: waveform, caches and jitter
    state are those of a plain receiver fed the genuine plain rows, but for STAT_MALFORMED of slot 1, which counts the three rejects"""
    from hilcodec_amd import dtx, jitter, synth
    from hilcodec_amd.graph_step import GraphedDecodeHop, GraphedEncodeHop
    from hilcodec_amd.jitter import JitterConfig
    from tests.hops import caches_equal
    B, n, m, K, hops = 4, 4, 1, 4, 14
    kw = dict(sessions=True, conceal=True, fec_stages=m, cng_order=K, jitter=JitterConfig(2, 8))
    rx = GraphedDecodeHop(speech, B, 1, n, DEV, srtp=srtp.SrtpConfig(), **kw)
    ref = GraphedDecodeHop(speech, B, 1, n, DEV, **kw)
    tx = GraphedEncodeHop(speech, B, HOP, n, DEV, sessions=True, header=True, fec_stages=m, dtx=dtx.DtxConfig(order=K))
    tb = wire.transport_bytes(n, m, 1)
    assert rx.tstride == tb and rx.wstride == wire.srtp_bytes(n, m, 1) and rx.arrivals.shape[1] == ref.arrivals.shape[1]
    sender, model = srtp.SenderModel(B, tb), srtp.ReceiverModel(B, tb)
    with pytest.raises(ValueError):
        rx.start(0)                                          # no key yet
    for b in range(B):
        for keyed in (rx, sender.keys, model.keys):
            keyed.set_key(b, *_key(3, b), ssrc=b + 1)
        rx.start(b)
        ref.start(b)
    x = synth.synth_clips(B, HOP * hops, seed=22).to(DEV)
    x[2, :, HOP * 4:HOP * 11] = 0
    history, rejects, count = [], 0, np.zeros(B, dtype=np.int64)
    for k in range(hops):
        pk, nb = tx.step(x[:, :, HOP * k:HOP * (k + 1)].contiguous())
        pk, nb = pk.cpu().numpy(), nb.cpu().numpy()
        prot = sender.protect(pk, nb)
        count += nb > 0
        plain = [(b, pk[b, :nb[b]].tobytes()) for b in range(B) if nb[b] > 0]
        wired = [(b, prot["packets"][b, :prot["nbytes"][b]].tobytes()) for b in range(B) if nb[b] > 0]
        history.append(dict(wired))
        if k == 6:
            p = history[6][1]
            forged = p[:5] + bytes([p[5] ^ 0x10]) + p[6:]
            wired = [(1, forged), (1, history[4][1]), (1, p[:12])] + wired      # in front of the genuine packet of the hop
            rejects = 3
        action = np.ones(B, dtype=np.int32) * (k == 0)
        arrays = []
        for rows, width in ((wired, tb + 10), (plain, tb)):
            data = np.zeros((len(rows), width), dtype=np.uint8)
            for a, (_, p) in enumerate(rows):
                data[a, :len(p)] = np.frombuffer(p, dtype=np.uint8)
            arrays.append(([s for s, _ in rows], torch.from_numpy(data), [len(p) for _, p in rows]))
        rec, offs = forward.arrival_records(arrays[0][0], arrays[0][1].numpy(), arrays[0][2], tb + 10, B, rx.max_arrivals)
        want = model.unprotect(rec, offs, action)
        a = rx.play(*arrays[0]).clone()
        b = ref.play(*arrays[1]).clone()
        assert torch.equal(a, b), k
        assert caches_equal(rx.cache_dec, ref.cache_dec) and torch.equal(rx.concealed, ref.concealed), k
        assert torch.equal(rx.cng_state, ref.cng_state), k
        assert np.array_equal(rx.srtp_state.cpu().numpy(), model.state), k
        assert np.array_equal(rx.arrivals[:len(wired)].cpu().numpy(), want[:len(wired)]), k
        js, jr = rx.jitter_state.cpu().numpy(), ref.jitter_state.cpu().numpy().copy()
        jr[1, jitter.STAT_MALFORMED] += rejects
        assert np.array_equal(js, jr), k
    st = model.state
    assert st[1, srtp.RX_AUTH_FAIL:srtp.RX_NOKEY].tolist() == [1, 1, 1] and not st[[0, 2, 3], srtp.RX_AUTH_FAIL:].any()
    assert st[:, srtp.RX_OK].tolist() == count.tolist() and count.min() > 8
    # a slot whose key is cleared rejects everything from the next hop on
    rx.clear_key(3)
    rx.play(*arrays[0])
    assert rx.srtp_state[3, srtp.RX_NOKEY] == 1 and rx.srtp_state[0, srtp.RX_REPLAY] == 1


def test_hop_constructor_and_accessor_errors(speech):
    from hilcodec_amd.graph_step import GraphedDecodeHop, GraphedEncodeHop
    from hilcodec_amd.jitter import JitterConfig
    cfg = srtp.SrtpConfig()
    for kw in (dict(header=True), dict(sessions=True)):
        with pytest.raises(ValueError):
            GraphedEncodeHop(speech, 2, HOP, 4, DEV, srtp=cfg, **kw)
    with pytest.raises(ValueError):
        GraphedEncodeHop(speech, 2, HOP, 4, DEV, sessions=True, header=True, srtp="AES")
    with pytest.raises(ValueError):
        GraphedDecodeHop(speech, 2, 1, 4, DEV, sessions=True, srtp=cfg)
    plain = GraphedEncodeHop(speech, 2, HOP, 4, DEV, sessions=True, header=True)
    for call in (lambda: plain.srtp_state, lambda: plain.set_key(0, bytes(16), bytes(14)), lambda: plain.clear_key(0)):
        with pytest.raises(RuntimeError):
            call()
    plain.start(0)                                           # no key needed without srtp
    rx = GraphedDecodeHop(speech, 2, 1, 4, DEV, sessions=True, jitter=JitterConfig(2, 4))
    for call in (lambda: rx.srtp_state, lambda: rx.set_key(0, bytes(16), bytes(14))):
        with pytest.raises(RuntimeError):
            call()
    rx.start(0)
