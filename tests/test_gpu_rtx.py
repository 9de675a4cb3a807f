"""GPU: NACK and retransmission of the graphed hops (GraphedDecodeHop(nack=NackConfig(...)), GraphedEncodeHop(rtx=RtxConfig(...))).
hilc_nack_build and hilc_rtx_step against rtx.py's models; the NACKing receiver against the receiver without NACKs and the
retransmitting sender against the sender without a history; the closed loop of tests/test_rtx_cpu.py with the real sender and
receiver — every comparison bit for bit (torch.equal / np.array_equal)."""
import numpy as np
import pytest
import torch

from hilcodec_amd import dtx, jitter, rtx, synth, wire
from hilcodec_amd.jitter import AdaptConfig, JitterConfig, JitterModel
from hilcodec_amd.rtx import NackConfig, NackModel, RtxConfig, RtxModel, nack_words
from hilcodec_amd.vbr import VbrConfig
from tests.hops import Network, arrival_arrays, arrival_records, caches_equal
from tests.rtx_loop import HOPS, LOOP_JITTER, LOOP_NACK, LOOP_RTX, Channel, bursts_of_two, singles_and_pairs

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
HOP = 320
ADAPT = AdaptConfig(window=8, resync=3, force_windows=2)
B_KERNEL = 5                                                 # a ragged last workgroup of the 4-slots-per-workgroup mapping


@pytest.fixture(scope="module")
def speech():
    return synth.streaming_model()


def dev(a, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).to(DEV)


# ---------------------------------------------------------------- hilc_nack_build against NackModel
NACK_CASES = [
    # (C, D, adaptive, n, T, m, K, NackConfig, seed)
    (4, 2, False, 4, 1, 0, None, NackConfig(1, 1, 2), 1),
    (8, 4, False, 8, 2, 1, 4, NackConfig(2, 1, 3, skip_fecable=True), 2),
    (32, 6, False, 8, 1, 1, 8, NackConfig(3, 2, 3), 3),
    (8, 3, True, 8, 2, 0, 8, NackConfig(2, 1, 255), 4),
]


@pytest.mark.parametrize("case", NACK_CASES, ids=lambda c: "C{}-D{}-adapt{}-n{}-T{}-m{}-K{}".format(*c[:7]))
def test_nack_build_kernel(case):
    """200 hops of Network traffic (losses, reordering, duplicates, SIDs, starts, holds, the 16-bit wrap) through the real jitter
    kernel; hilc_nack_build on its rows against NackModel on JitterModel's, which are asserted equal first"""
    from hilcodec_amd import ops
    C, D, adaptive, n, T, m, K, ncfg, seed = case
    B, hops = B_KERNEL, 200
    cfg = JitterConfig(D, C, adapt=ADAPT if adaptive else None)
    jm, nm = JitterModel(B, cfg, n, m, T, K, True), NackModel(B, ncfg, C, m)
    net = Network(B, n, m, K, T, seed=seed, loss=0.12, delay=min(D + 1, 4), dup=0.03, bad=0.01, hold=0.03, start=0.01,
                  sid=0.04 if K is not None else 0.0, every=1 << 30, mild=False)
    net.h[:2] = 65450                                        # these cross the 16-bit wrap
    stride = wire.packet_bytes(n + m, T)
    ints = dict(dtype=torch.int32, device=DEV)
    state, meta = torch.zeros(B, jitter.ST_WORDS, **ints), torch.zeros(B, C, **ints)
    ring, adapt = torch.zeros(B, C, (stride + 3) // 4, **ints), torch.zeros(B, jitter.AD_WORDS, **ints)
    jrows, pk = torch.zeros(3, B, **ints), torch.zeros(B, stride, dtype=torch.uint8, device=DEV)
    rows = torch.zeros(B, rtx.NK_WORDS, **ints)
    nacks = torch.zeros(B, 4, dtype=torch.uint8, device=DEV)
    due = torch.full((B,), -9, **ints)
    retried = cleared = wide = 0
    for k in range(hops):
        slots, packets, nbytes, action, hold = net.hop()
        arr, offs = arrival_records(slots, packets, nbytes, net.tbytes, B, 8 * B)
        args = (arr, offs, dev(hold), jrows[0], pk, state, meta, ring)
        kw = dict(action=dev(action), lost=jrows[1], fec=jrows[2] if m else None)
        if adaptive:
            ops.jitter_adapt_step(*args, adapt, n, m, T, K, cfg, **kw)
        else:
            ops.jitter_step(*args, n, m, T, K, D, **kw)
        jm.step(action, hold, slots, packets, nbytes)
        assert np.array_equal(state.cpu().numpy(), jm.state) and np.array_equal(meta.cpu().numpy(), jm.meta), k
        cleared += int(((action != 0) & nm.state.any(axis=1)).sum())
        want = nm.step(jm.state, jm.meta, action)
        ops.nack_build(state, meta, rows, nacks, due, ncfg, m, action=dev(action))
        assert np.array_equal(rows.cpu().numpy(), nm.state), k
        assert np.array_equal(nacks.cpu().numpy(), want["nacks"]), k
        assert np.array_equal(due.cpu().numpy(), want["due"]), k
        assert np.array_equal(state.cpu().numpy(), jm.state) and np.array_equal(meta.cpu().numpy(), jm.meta), k      # read only
        words = nm.state[:, rtx.NK_RING:].astype(np.int64) & 0xFFFFFFFF
        retried += int((((words >> 16) & 255) >= 2).sum())
        wide += int(sum(want["due"][b] and wire.parse_nack(want["nacks"][b])[1] != 0 for b in range(B)))
    st = nm.state
    assert all(st[:, i].sum() > 0 for i in range(rtx.NK_RING)), st[:, :rtx.NK_RING]
    assert cleared >= 1 and wide >= 1 and (retried >= 1 or C == 4)      # in a ring of 4 a hole expires before its second request
    assert not st[:, rtx.NK_RING + C:].any()
    # without an action row no slot is cleared
    ops.nack_build(state, meta, rows, nacks, due, ncfg, m)
    nm.step(jm.state, jm.meta, np.zeros(B, dtype=np.int32))
    assert np.array_equal(rows.cpu().numpy(), nm.state)


# ---------------------------------------------------------------- hilc_rtx_step against RtxModel
@pytest.mark.parametrize("R,P,n,T,m", [(2, 1, 4, 1, 1), (4, 2, 4, 2, 0), (16, 2, 8, 2, 1), (16, 1, 8, 1, 0)])
def test_rtx_step_kernel(R, P, n, T, m):
    from hilcodec_amd import ops
    B, hops = B_KERNEL, 200
    tb = wire.transport_bytes(n, m, T)
    assert tb % 4 != 0
    cfg = RtxConfig(R, P)
    model = RtxModel(B, cfg, tb)
    rng = np.random.default_rng(100 * R + P)
    ints = dict(dtype=torch.int32, device=DEV)
    tags, ring, rows = torch.zeros(B, R, **ints), torch.zeros(B, R, (tb + 3) // 4, **ints), torch.zeros(B, rtx.RX_WORDS, **ints)
    out, out_nb = torch.zeros(B, P, tb, dtype=torch.uint8, device=DEV), torch.zeros(B, P, **ints)
    h = rng.integers(0, 65536, B)
    h[0] = 65500                                             # crosses the 16-bit wrap
    lengths = [wire.TRANSPORT_HEADER + wire.packet_bytes(k, T) for k in range(1, n + m + 1)] + [wire.TRANSPORT_HEADER + 1]
    for k in range(hops):
        action = (rng.random(B) < 0.03).astype(np.int32) * rng.choice([-1, 1, 3], B).astype(np.int32)
        h[action != 0] = 0
        packets = rng.integers(0, 256, (B, tb), dtype=np.uint8)       # garbage past the byte count: the history masks it
        nbytes = np.where(rng.random(B) < 0.8, rng.choice(lengths, B), 0).astype(np.int32)
        words = np.zeros((B, 2), dtype=np.int64)
        for b in range(B):
            packets[b, 0], packets[b, 1] = h[b] >> 8, h[b] & 255
            if nbytes[b]:
                h[b] = (h[b] + 1) & 0xFFFF
            if rng.random() < 0.5:
                how = rng.random()
                base = (h[b] - int(rng.integers(0, R + 3))) & 0xFFFF if how < 0.85 else int(rng.integers(0, 65536))
                bitmap = int(rng.integers(0, 65536)) if how < 0.3 else int(rng.integers(0, 8)) if how < 0.7 else 0
                words[b] = nack_words(base, bitmap)
        want = model.step(packets, nbytes, words, action)
        out.fill_(0xEE)
        out_nb.fill_(-9)
        d_pk = dev(packets, np.uint8)
        ops.rtx_step(d_pk, dev(nbytes), tags, ring, rows, out, out_nb, nack_base=dev(words[:, 0]), nack_bitmap=dev(words[:, 1]),
                     action=dev(action))
        assert np.array_equal(out.cpu().numpy(), want["packets"]), k
        assert np.array_equal(out_nb.cpu().numpy(), want["nbytes"]), k
        assert np.array_equal(tags.cpu().numpy(), model.tags) and np.array_equal(rows.cpu().numpy(), model.state), k
        got = ring.cpu().numpy().view(np.uint8).reshape(B, R, -1)
        assert np.array_equal(got[:, :, :tb], model.ring) and not got[:, :, tb:].any(), k
        assert np.array_equal(d_pk.cpu().numpy(), packets), k
    assert all(model.state[:, i].sum() > 0 for i in range(rtx.RX_WORDS)), model.state
    # no NACK rows, no action row: the hop is stored, the rows are zero
    model.step(packets, nbytes)
    ops.rtx_step(d_pk, dev(nbytes), tags, ring, rows, out, out_nb)
    assert np.array_equal(tags.cpu().numpy(), model.tags) and np.array_equal(rows.cpu().numpy(), model.state)
    assert not out.any() and not out_nb.any()


def test_entry_points_refuse_bad_arguments():
    from hilcodec_amd import _lib, ops
    lib = _lib.lib
    NULL, SHAPE, RANGE = -2, -1, -5
    z = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt, device=DEV)
    B, C = 2, 8
    js, meta, rows, nacks, due = z(B, jitter.ST_WORDS), z(B, C), z(B, rtx.NK_WORDS), z(B, 4, dt=torch.uint8), z(B)
    p = lambda t: t.data_ptr()
    good = [p(js), p(meta), None, p(rows), p(nacks), p(due), B, C, 0, 2, 3, 2, 0, None]
    assert lib.hilc_nack_build(*good) == 0
    for i in (0, 1, 3, 4, 5):
        assert lib.hilc_nack_build(*[None if j == i else v for j, v in enumerate(good)]) == NULL, i
    for i, v, code in ((6, 0, SHAPE), (7, 3, RANGE), (7, 6, RANGE), (7, 64, RANGE), (7, 1, RANGE), (8, -1, RANGE), (9, 0, RANGE),
                       (9, 31, RANGE), (10, 0, RANGE), (10, 256, RANGE), (11, 0, RANGE), (11, 256, RANGE)):
        assert lib.hilc_nack_build(*[v if j == i else w for j, w in enumerate(good)]) == code, (i, v)
    torch.cuda.synchronize()
    assert not rows.any() and not due.any()                  # an unanchored slot does nothing; a refused call launches nothing
    tb, R, P = 13, 4, 2
    pk, nb, base, bits = z(B, tb, dt=torch.uint8), z(B), z(B), z(B)
    tags, ring, rx, out, onb = z(B, R), z(B, R, 4), z(B, rtx.RX_WORDS), z(B, P, tb, dt=torch.uint8), z(B, P)
    good = [p(pk), p(nb), p(base), p(bits), None, p(tags), p(ring), p(rx), p(out), p(onb), B, tb, R, P, None]
    assert lib.hilc_rtx_step(*good) == 0
    for i in (0, 1, 2, 3, 5, 6, 7, 8, 9):                    # one NACK row without the other is refused too
        assert lib.hilc_rtx_step(*[None if j == i else v for j, v in enumerate(good)]) == NULL, i
    for i, v, code in ((10, 0, SHAPE), (11, 3, SHAPE), (11, 1 << 15, SHAPE), (12, 3, RANGE), (12, 1, RANGE), (12, 128, RANGE),
                       (13, 0, RANGE), (13, 5, RANGE)):
        assert lib.hilc_rtx_step(*[v if j == i else w for j, w in enumerate(good)]) == code, (i, v)
    # the ops check the widths of their rows
    cfg = NackConfig()
    for bad in ((z(B, 13), meta, rows, nacks, due), (js, meta, z(B, rtx.NK_WORDS - 1), nacks, due), (js, meta, rows, z(B, 3, dt=torch.uint8), due),
                (js, z(B + 1, C), rows, nacks, due)):
        with pytest.raises(RuntimeError):
            ops.nack_build(*bad, cfg)
    with pytest.raises(AssertionError):
        ops.nack_build(js, z(B, 6), rows, nacks, due, cfg)   # capacity no power of two: HILC_ERR_RANGE
    for bad in ((pk, nb, tags, z(B, R, 3), rx, out, onb), (pk, nb, tags, ring, z(B, 4), out, onb), (pk, nb, tags, ring, rx, z(B, P, tb + 1, dt=torch.uint8), onb),
                (pk, nb, tags, ring, rx, out, z(B, P + 1)), (pk, z(B + 1), tags, ring, rx, out, onb)):
        with pytest.raises(RuntimeError):
            ops.rtx_step(*bad)
    with pytest.raises(AssertionError):
        ops.rtx_step(pk, nb, z(B, 3), z(B, 3, 4), rx, out, onb)      # history 3
    with pytest.raises((AssertionError, RuntimeError)):
        ops.rtx_step(pk, nb, tags, ring, rx, z(B, 0, tb, dt=torch.uint8), z(B, 0))      # per_hop 0: no rows to write to


# ---------------------------------------------------------------- the receiver graph
def test_nacking_receiver_only_observes(speech):
    from hilcodec_amd.graph_step import GraphedDecodeHop
    B, n, m, K, hops = 4, 8, 1, 8, 80
    cfg, ncfg = JitterConfig(3, 8, adapt=ADAPT), NackConfig(2, 2, 2)
    kw = dict(sessions=True, conceal=True, fec_stages=m, cng_order=K, jitter=cfg)
    rx = GraphedDecodeHop(speech, B, 1, n, DEV, nack=ncfg, **kw)
    ref = GraphedDecodeHop(speech, B, 1, n, DEV, **kw)
    jm, nm = JitterModel(B, cfg, n, m, 1, K, True), NackModel(B, ncfg, 8, m)
    net = Network(B, n, m, K, 1, seed=6, loss=0.12, delay=3, dup=0.02, bad=0.02, hold=0.03, sid=0.05, restart=0.01, every=10, mild=False)
    for k in range(hops):
        slots, packets, nbytes, action, hold = net.hop()
        if k == 50:
            assert nm.state[2].any()
            action[2] = 1                                    # a start in the middle clears the slot's NACK row
        for b in np.nonzero(action)[0]:
            rx.start(int(b))
            ref.start(int(b))
        jm.step(action, hold, slots, packets, nbytes)
        want = nm.step(jm.state, jm.meta, action)
        held = np.nonzero(hold)[0].tolist()
        a = rx.play(slots, torch.from_numpy(packets), nbytes, hold=held).clone()
        b = ref.play(slots, torch.from_numpy(packets), nbytes, hold=held).clone()
        assert torch.equal(a, b), k
        assert caches_equal(rx.cache_dec, ref.cache_dec), k
        for name in ("jitter_state", "jitter_adapt", "concealed", "cng_state"):
            assert torch.equal(getattr(rx, name), getattr(ref, name)), (name, k)
        assert np.array_equal(rx.jitter_state.cpu().numpy(), jm.state), k
        assert np.array_equal(rx.nacks.cpu().numpy(), want["nacks"]), k
        assert np.array_equal(rx.nack_due.cpu().numpy(), want["due"]), k
        assert np.array_equal(rx.nack_state.cpu().numpy(), nm.state), k
    assert (nm.state[:, rtx.NK_SENT] > 0).all() and jm.state[:, jitter.STAT_LOST].sum() > 0
    # a start of every slot with no arrival on that hop: every NACK row, NACK and flag is zero
    assert rx.nack_state.any() and rx.nacks.any()
    for b in range(B):
        rx.start(b)
    rx.play([], torch.zeros(0, rx.tstride, dtype=torch.uint8), [])
    assert not rx.nack_state.any() and not rx.nacks.any() and not rx.nack_due.any()


# ---------------------------------------------------------------- the sender graph
@pytest.mark.parametrize("variant", ["header", "fec-vbr-dtx"])
def test_retransmitting_sender_only_observes(speech, variant):
    from hilcodec_amd.graph_step import GraphedEncodeHop
    B, n, hops = 3, 4, 24
    kw = dict(sessions=True, header=True)
    if variant != "header":
        kw.update(fec_stages=1, vbr=VbrConfig(3.0, n_min=1), dtx=dtx.DtxConfig(order=4))
    tx = GraphedEncodeHop(speech, B, HOP, n, DEV, rtx=RtxConfig(8, 2), **kw)
    ref = GraphedEncodeHop(speech, B, HOP, n, DEV, **kw)
    tb = wire.transport_bytes(n, kw.get("fec_stages", 0), 1)
    model = RtxModel(B, RtxConfig(8, 2), tb)
    x = synth.synth_clips(B, HOP * hops, seed=12).to(DEV)
    x[1, :, HOP * 8:HOP * 18] = 0                            # with DTX: SIDs and silence on slot 1
    for k in range(hops):
        action = np.zeros(B, dtype=np.int32)
        if k == 10:
            tx.start(2)
            ref.start(2)
            action[2] = -1
        holds = [0] if k in (5, 6) else []
        xk = x[:, :, HOP * k:HOP * (k + 1)].contiguous()
        (pk, nb), (pk1, nb1) = tx.step(xk, hold=holds), ref.step(xk, hold=holds)
        assert torch.equal(pk, pk1) and torch.equal(nb, nb1) and torch.equal(tx.indices, ref.indices), k
        assert caches_equal(tx.cache_enc, ref.cache_enc) and torch.equal(tx.hop_index, ref.hop_index), k
        if variant != "header":
            assert torch.equal(tx.kind, ref.kind) and torch.equal(tx.n_eff, ref.n_eff) and torch.equal(tx.distortion, ref.distortion), k
        assert not tx.rtx_nbytes.any() and not tx.rtx_packets.any(), k
        model.step(pk.cpu().numpy(), nb.cpu().numpy(), None, action)
        assert np.array_equal(tx.rtx_state.cpu().numpy(), model.state), k
    if variant == "header":
        assert model.state[:, rtx.RX_STORED].tolist() == [hops - 2, hops, hops]      # held hops store nothing
    else:
        assert model.state[1, rtx.RX_STORED] < hops          # nor do SILENT hops
    # the history is what was sent: the last hops come back byte for byte, and reset clears every history
    h_last = [int(v) - 1 for v in tx.hop_index.tolist()]
    tx.step(xk, hold=[0, 1, 2], nacks=([0, 1, 2], [wire.pack_nack(h & 0xFFFF, 0) for h in h_last]))
    want = model.step(np.zeros((B, tb), dtype=np.uint8), [0] * B, [nack_words(h & 0xFFFF, 0) for h in h_last])
    assert np.array_equal(tx.rtx_packets.cpu().numpy(), want["packets"]) and np.array_equal(tx.rtx_nbytes.cpu().numpy(), want["nbytes"])
    assert int(nb[2]) > 0 and tx.rtx_nbytes[2, 0] == nb[2] and torch.equal(tx.rtx_packets[2, 0], pk[2])
    tx.reset()
    assert not tx.rtx_state.any() and not tx.rtx_nbytes.any()
    tx.step(xk, nacks=([0], [wire.pack_nack(h_last[0] & 0xFFFF, 0)]))
    assert tx.rtx_state[0].tolist() == [1, 1, 0, 1, 0]


def test_sessions_start_hold_and_stop(speech):
    """a start makes a NACK for the slot's earlier hops a MISS and leaves its neighbours' histories intact; a held slot still answers;
    stop keeps the history"""
    from hilcodec_amd.graph_step import GraphedEncodeHop
    B, n, T = 3, 8, 2
    tx = GraphedEncodeHop(speech, B, HOP * T, n, DEV, sessions=True, header=True, rtx=RtxConfig(8, 2))
    x = synth.synth_clips(B, HOP * T * 12, seed=3).to(DEV)
    sent = []
    step = lambda k, **kw: tx.step(x[:, :, HOP * T * k:HOP * T * (k + 1)].contiguous(), **kw)
    for k in range(6):
        pk, nb = step(k)
        sent.append((pk.cpu().clone(), nb.cpu().clone()))
    assert tx.rtx_packets.shape[2] == wire.transport_bytes(n, 0, T) == 23
    ask = lambda *hops: wire.pack_nack(hops[0], sum(1 << (h - hops[0] - 1) for h in hops[1:]))
    tx.start(0)
    tx.stop(2)
    step(6, hold=[1], nacks=(torch.tensor([0, 1, 2]), torch.tensor([list(ask(3)), list(ask(2, 4)), list(ask(5, 1 + 5))], dtype=torch.uint8)))
    got, got_nb = tx.rtx_packets.cpu(), tx.rtx_nbytes.cpu()
    assert got_nb.tolist() == [[0, 0], [23, 23], [23, 0]] and not got[0].any()
    assert torch.equal(got[1, 0], sent[2][0][1]) and torch.equal(got[1, 1], sent[4][0][1]) and torch.equal(got[2, 0], sent[5][0][2])
    # slot 0: stored hop 0 of its new stream, one request, one miss; slot 1 (held): nothing stored; slot 2 (stopped): hop 6 never sent
    assert tx.rtx_state.cpu().tolist() == [[7, 1, 0, 1, 0], [6, 1, 2, 0, 0], [6, 1, 1, 1, 0]]
    # the new stream's hop 0 is in slot 0's history, hop 3 still is not; a NACK applies to exactly one hop
    step(7, nacks=([0, 0], [ask(5), ask(0, 3)]))             # named twice: the last one counts
    assert tx.rtx_nbytes.cpu().tolist() == [[23, 0], [0, 0], [0, 0]] and tx.rtx_state[0].tolist() == [8, 2, 1, 2, 0]
    step(8)
    assert not tx.rtx_nbytes.any() and tx.rtx_state[:, rtx.RX_REQUESTS].tolist() == [2, 1, 1]


# ---------------------------------------------------------------- end to end
def test_closed_loop_with_the_real_hops(speech):
    """the closed loop of tests/test_rtx_cpu.py with the real sender and receiver: slot 0 loses 40 singles and pairs, slot 1 22 bursts
    of two, slot 2 nothing.  With NACK and retransmission the waveform is the lossless receiver's on every hop; without, it is not."""
    from hilcodec_amd.graph_step import GraphedDecodeHop, GraphedEncodeHop
    B, n = 3, 8
    drops = {0: singles_and_pairs(), 1: bursts_of_two()}
    tx = GraphedEncodeHop(speech, B, HOP, n, DEV, sessions=True, header=True, rtx=LOOP_RTX)
    kw = dict(sessions=True, jitter=LOOP_JITTER, conceal=True, max_arrivals=B * (1 + LOOP_RTX.per_hop))
    rx = GraphedDecodeHop(speech, B, 1, n, DEV, nack=LOOP_NACK, **kw)
    ref = GraphedDecodeHop(speech, B, 1, n, DEV, nack=LOOP_NACK, **kw)       # the same receiver on a lossless channel
    bare = GraphedDecodeHop(speech, B, 1, n, DEV, **kw)                      # the lossy channel without NACKs
    tb = rx.tstride
    assert tb == wire.transport_bytes(n, 0, 1) == 13
    ch = Channel(drops, LOOP_NACK.rtt_hops)

    def play(hop, arrived):
        slots, packets, nbytes = arrival_arrays(arrived, tb)
        return hop.play(slots, torch.from_numpy(packets), nbytes)

    x = (torch.randn(B, 1, HOPS * HOP, generator=torch.Generator().manual_seed(9)) * 0.1).to(DEV)
    differ = 0
    for t in range(HOPS):
        pk, nb = tx.step(x[:, :, HOP * t:HOP * (t + 1)].contiguous(), nacks=ch.nacks_for(t))
        pk, nb = pk.cpu().numpy(), nb.cpu().numpy()
        rp, rn = tx.rtx_packets.cpu().numpy(), tx.rtx_nbytes.cpu().numpy()
        first = [(b, pk[b, :nb[b]].tobytes()) for b in range(B)]
        again = [(b, rp[b, q, :rn[b, q]].tobytes()) for b in range(B) for q in range(LOOP_RTX.per_hop) if rn[b, q] > 0]
        wav = play(rx, ch.arrivals(t, first, again))
        want = play(ref, first)
        assert torch.equal(wav, want), t
        differ += int(not torch.equal(play(bare, ch.arrivals(t, first, [])), want))
        due, blobs = rx.nack_due.cpu().numpy(), rx.nacks.cpu().numpy()
        ch.push_nacks(t, [(b, blobs[b].tobytes()) for b in range(B) if due[b]])
    js, js_ref, js_bare = (h.jitter_state.cpu().numpy() for h in (rx, ref, bare))
    assert js[:, jitter.STAT_LOST].tolist() == [0, 0, 0] and js_ref[:, jitter.STAT_LOST].tolist() == [0, 0, 0]
    assert js_bare[:, jitter.STAT_LOST].tolist() == [40, 44, 0] and differ > 0
    assert caches_equal(rx.cache_dec, ref.cache_dec)
    nk = rx.nack_state.cpu().numpy()
    assert nk[:, rtx.NK_ASKED].tolist() == [40, 44, 0]
    assert tx.rtx_state.cpu().numpy().tolist() == [[HOPS, nk[0, rtx.NK_SENT], 40, 0, 0], [HOPS, nk[1, rtx.NK_SENT], 44, 0, 0], [HOPS, 0, 0, 0, 0]]
    # slot 2 is undisturbed: the rows of the run where nobody loses anything
    assert np.array_equal(js[2], js_ref[2]) and np.array_equal(nk[2], ref.nack_state.cpu().numpy()[2]) and not nk[2].any()


# ---------------------------------------------------------------- accessors and constructor errors
def test_accessors_and_constructor_errors(speech):
    from hilcodec_amd.graph_step import GraphedDecodeHop, GraphedEncodeHop
    jc = JitterConfig(2, 8)
    with pytest.raises(ValueError):
        GraphedDecodeHop(speech, 2, 1, 8, DEV, sessions=True, nack=NackConfig())                      # needs jitter
    with pytest.raises(ValueError):
        GraphedDecodeHop(speech, 2, 1, 8, DEV, sessions=True, jitter=jc, nack=RtxConfig())
    plain = GraphedDecodeHop(speech, 2, 1, 8, DEV, sessions=True, jitter=jc)
    for name in ("nacks", "nack_due", "nack_state"):
        with pytest.raises(RuntimeError):
            getattr(plain, name)
    rx = GraphedDecodeHop(speech, 2, 1, 8, DEV, sessions=True, jitter=jc, nack=NackConfig())
    assert rx.nacks.shape == (2, 4) and rx.nacks.dtype == torch.uint8 and rx.nacks.is_cuda
    assert rx.nack_due.shape == (2,) and rx.nack_due.dtype == torch.int32
    assert rx.nack_state.shape == (2, rtx.NK_WORDS) and rx.nack_state.dtype == torch.int32

    cfg = RtxConfig(4, 2)
    with pytest.raises(ValueError):
        GraphedEncodeHop(speech, 2, HOP, 8, DEV, header=True, rtx=cfg)                                # needs sessions
    with pytest.raises(ValueError):
        GraphedEncodeHop(speech, 2, HOP, 8, DEV, sessions=True, rtx=cfg)                              # needs header
    with pytest.raises(ValueError):
        GraphedEncodeHop(speech, 2, HOP, 8, DEV, sessions=True, header=True, rtx=NackConfig())
    x = torch.zeros(2, 1, HOP, device=DEV)
    plain = GraphedEncodeHop(speech, 2, HOP, 8, DEV, sessions=True, header=True)
    for name in ("rtx_packets", "rtx_nbytes", "rtx_state"):
        with pytest.raises(RuntimeError):
            getattr(plain, name)
    with pytest.raises(RuntimeError):
        plain.step(x, nacks=([0], [b"\x00\x00\x00\x00"]))
    tx = GraphedEncodeHop(speech, 2, HOP, 8, DEV, sessions=True, header=True, fec_stages=1, rtx=cfg)
    tb = wire.transport_bytes(8, 1, 1)
    assert tx.rtx_packets.shape == (2, 2, tb) and tx.rtx_packets.dtype == torch.uint8 and tx.rtx_packets.is_cuda
    assert tx.rtx_nbytes.shape == (2, 2) and tx.rtx_nbytes.dtype == torch.int32
    assert tx.rtx_state.shape == (2, rtx.RX_WORDS) and tx.rtx_state.dtype == torch.int32
    for bad in (([2], [b"abcd"]), ([-1], [b"abcd"]), ([0], [b"abc"]), ([0], [b"abcde"]), ([0, 1], [b"abcd"]),
                ([0], torch.zeros(1, 3, dtype=torch.uint8)), ([0], torch.zeros(1, 4, dtype=torch.int32)), [0]):
        with pytest.raises(ValueError):
            tx.step(x, nacks=bad)
    assert not tx.rtx_state.any()                            # nothing was launched
    # a step that raises before its upload (a wrong input shape) drops its NACKs: the next hop does not apply them
    with pytest.raises(RuntimeError):
        tx.step(torch.zeros(2, 1, HOP + 1, device=DEV), nacks=([0], [wire.pack_nack(0, 0)]))
    tx.step(x)
    assert tx.rtx_state.cpu().tolist() == [[1, 0, 0, 0, 0], [1, 0, 0, 0, 0]]
