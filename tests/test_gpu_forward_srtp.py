"""GPU: SRTP on the forwarding hop (GraphedForwardHop(srtp=SrtpConfig())).  hilc_srtp_protect_routes against forward_srtp.RouteModel bit
for bit — rows, byte counts and route rows; ragged workgroups, the word and the byte path, 4-byte-skewed views, the wrap, reordered and
repeated SEQs, restarts, listeners without a key, an exhausted route — then the protected hop against the plain hop fed the same
plaintext, with ForwarderModel beside it and the listeners' clients decrypting what it returns.  Every comparison is exact."""
import numpy as np
import pytest
import torch

from hilcodec_amd import audio_level, downlink, forward, forward_srtp, rate, srtp, wire
from hilcodec_amd.forward_srtp import MAX_EPOCH, RT_EPOCH, RT_EXHAUSTED, RT_NOKEY, RT_PROTECTED, RT_ROC, RT_SEEN, RT_SL, RT_STALE
from tests.alignment import skew
from tests.forward_loop import Membership
from tests.forward_srtp_loop import Call, Clients, forge, key
from tests.hops import SRTP_LENGTHS as LENGTHS
from tests.hops import arrival_arrays

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def dev(a, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).to(DEV)


# ---------------------------------------------------------------- the kernel
@pytest.mark.parametrize("tb, views", [(80, False), (80, True), (41, False), (41, True), (78, False), (78, True)],
                         ids=["word", "word-skewed", "byte", "byte-skewed", "out-aligned", "out-aligned-skewed"])
@pytest.mark.parametrize("B, F, P", [(23, 3, 3), (5, 8, 4), (67, 1, 1)], ids=["23x3x3", "5x8x4", "67x1x1"])
def test_protect_routes_kernel(B, F, P, tb, views):
    """8 hops against RouteModel.  (23, 3, 3): 207 rows, 3 does not divide 64 (lanes 63 idle) and the last workgroup is partial;
    (5, 8, 4): full bursts, 16 routes per workgroup; (67, 1, 1): one row per route, two workgroups.  Route rows start at SEQ 0xFFFE so
    that the run crosses the wrap; a row's SEQ is the route's next one, or one from a few rows back (late, or a repeat), byte counts
    come from every AES and SHA-1 edge; random restart flags of every kind; two listeners have no key; one route starts at MAX_EPOCH;
    the outputs are pre-filled, so every byte must be written"""
    from hilcodec_amd import ops
    rng = np.random.default_rng(1000 * B + 10 * tb + views)
    model = forward_srtp.RouteModel(B, F, P, tb)
    unkeyed = (1, B - 1)
    for b in range(B):
        if b not in unkeyed:
            model.keys.set_key(b, rng.integers(0, 256, 16, dtype=np.uint8).tobytes(), rng.integers(0, 256, 14, dtype=np.uint8).tobytes(),
                               ssrc=int(rng.integers(0, 1 << 32)))
    keys = dev(model.keys.rows)
    model.state[:, :, RT_SL], model.state[:, :, RT_SEEN] = 0xFFFE, 1
    model.state[0, 0, RT_ROC] = -1                           # 2^32 - 1: the counter wraps, too
    model.state[2, F - 1, RT_EPOCH] = MAX_EPOCH              # its first restart exhausts it
    model.state[3, 0, RT_EPOCH] = MAX_EPOCH - 1
    rt = dev(model.state)
    nxt = np.full((B, F), 0xFFFF, dtype=np.int64)
    out = torch.full((B, F, P, tb + 10), 0xAB, dtype=torch.uint8, device=DEV)
    out_nb = torch.full((B, F, P), -9, dtype=torch.int32, device=DEV)
    lengths, wrapped = set(), False
    for h in range(8):
        rows = rng.integers(0, 256, (B, F, P, tb), dtype=np.uint8)
        nbytes = np.minimum(np.array(LENGTHS)[rng.integers(0, len(LENGTHS), (B, F, P))], tb).astype(np.int32)
        for b in range(B):
            for j in range(F):
                for k in range(P):
                    seq = nxt[b, j]
                    if rng.random() < 0.25:
                        seq = (nxt[b, j] - int(rng.integers(1, 6))) & 0xFFFF             # late or repeated
                    elif nbytes[b, j, k] >= 3:
                        nxt[b, j] = (nxt[b, j] + 1) & 0xFFFF
                    rows[b, j, k, 0], rows[b, j, k, 1] = seq >> 8, seq & 255
        routes = rng.integers(-1, B, (B, F)).astype(np.int32)
        new_routes = (rng.random((B, F)) < 0.08).astype(np.int32) * (h > 0)
        new_routes[2, F - 1] = h == 3
        flags = [(rng.random(B) < 0.05).astype(np.int32) * (h > 0) * rng.choice([-1, 1, 3], B).astype(np.int32) for _ in range(3)]
        if h == 5:
            routes[0, 0] = B + 3                             # an owner outside [0, B) is no owner: nothing is read for it
        want = model.protect(rows, nbytes, routes, new_routes, *flags)
        args = [dev(rows, np.uint8), dev(nbytes), dev(routes), dev(new_routes), keys, rt, out, out_nb] + [dev(f) for f in flags]
        if views:
            args = [skew(t, 1 + (i + h) % 3) for i, t in enumerate(args)]
        ops.srtp_protect_routes(*args[:6], out=args[6], out_nbytes=args[7], action=args[8], rekey_up=args[9], rekey_down=args[10])
        if views:
            rt.copy_(args[5])
        assert np.array_equal(args[7].cpu().numpy(), want["out_nbytes"]), h
        assert np.array_equal(args[6].cpu().numpy(), want["out"]), h
        assert np.array_equal(rt.cpu().numpy(), model.state), h
        assert np.array_equal(args[0].cpu().numpy(), rows) and np.array_equal(args[1].cpu().numpy(), nbytes)          # read only
        lengths |= set(nbytes[want["out_nbytes"] > 0].tolist())
        wrapped = wrapped or bool((model.state[:, :, RT_ROC] == 1).any())
    st = model.state
    keyed = [b for b in range(B) if b not in unkeyed]
    assert lengths == set(min(v, tb) for v in LENGTHS if v >= 3)
    assert st[list(unkeyed), :, RT_NOKEY].min() >= 1 and not st[list(unkeyed), :, RT_PROTECTED].any()
    assert st[keyed][:, :, RT_PROTECTED].sum() > st[keyed][:, :, RT_STALE].sum() > 0
    assert st[2, F - 1, RT_SEEN] == forward_srtp.SEEN_EXHAUSTED and st[2, F - 1, RT_EXHAUSTED] >= 1 and st[2, F - 1, RT_EPOCH] == MAX_EPOCH
    assert wrapped and st[:, :, RT_EPOCH].max() == MAX_EPOCH and (st[keyed][:, :, RT_EPOCH] >= 1).any()
    # without the optional rows nothing restarts but what new_routes names; outputs are allocated
    rows[:, :, :, 0], rows[:, :, :, 1] = 0x7F, np.arange(P, dtype=np.uint8)
    none = np.zeros((B, F), dtype=np.int32)
    want = model.protect(rows, nbytes, routes, none)
    got, got_nb = ops.srtp_protect_routes(dev(rows, np.uint8), dev(nbytes), dev(routes), dev(none), keys, rt)
    assert np.array_equal(got.cpu().numpy(), want["out"]) and np.array_equal(got_nb.cpu().numpy(), want["out_nbytes"])
    assert np.array_equal(rt.cpu().numpy(), model.state)


def test_argument_checks():
    from hilcodec_amd import ops
    B, F, P, tb = 3, 2, 2, 20
    ints = dict(dtype=torch.int32, device=DEV)
    good = dict(rows=torch.zeros(B, F, P, tb, dtype=torch.uint8, device=DEV), nbytes=torch.zeros(B, F, P, **ints),
                routes=torch.zeros(B, F, **ints), new_routes=torch.zeros(B, F, **ints), keys=torch.zeros(B, srtp.KEY_WORDS, **ints),
                route_rows=torch.zeros(B, F, forward_srtp.RT_WORDS, **ints))
    ops.srtp_protect_routes(**good)
    row = torch.zeros(B, **ints)
    for bad in (dict(rows=good["rows"][0]), dict(nbytes=good["nbytes"][:, :, :1].contiguous()), dict(routes=good["routes"][:2]),
                dict(new_routes=good["new_routes"][:, :1].contiguous()), dict(keys=good["keys"][:, :-1].contiguous()),
                dict(route_rows=good["route_rows"][:, :, :-1].contiguous()), dict(route_rows=torch.zeros(B, srtp.TX_WORDS, **ints)),
                dict(out=torch.zeros(B, F, P, tb, dtype=torch.uint8, device=DEV)), dict(out_nbytes=torch.zeros(B, F, **ints)),
                dict(action=row[:2]), dict(rekey_up=row[:2]), dict(rekey_down=torch.zeros(B + 1, **ints)),
                dict(nbytes=good["nbytes"].long()), dict(rows=good["rows"].int()), dict(keys=good["keys"].float()),
                dict(rows=torch.zeros(B, F, P, 3, dtype=torch.uint8, device=DEV)),                     # no room behind the header
                dict(rows=torch.zeros(B, F, 5, tb, dtype=torch.uint8, device=DEV), nbytes=torch.zeros(B, F, 5, **ints)),  # burst > 4
                dict(rows=good["rows"].transpose(1, 2), nbytes=good["nbytes"].transpose(1, 2))):
        with pytest.raises(RuntimeError):
            ops.srtp_protect_routes(**{**good, **bad})
    with pytest.raises(RuntimeError):
        ops.srtp_protect_routes(**{k: v.cpu() for k, v in good.items()})
    with pytest.raises(RuntimeError):
        ops.srtp_protect_routes(**{**good, "action": row.cpu()})


# ---------------------------------------------------------------- the hop
B_HOP, N, T, M, K = 16, 4, 1, 1, 4
CFG = forward.ForwardConfig(fanout=2, burst=2, hang_hops=3)


@pytest.mark.parametrize("speakers, rated", [(False, False), (True, False), (False, True)], ids=["plain", "speakers", "rate"])
def test_protected_hop_against_the_plain_hop_and_the_model(speakers, rated):
    """16 slots in rooms of 4, 40 hops.  A GraphedForwardHop(srtp=) is fed what the senders protect, a plain one the plaintext: every
    row the first returns, decrypted by the listeners' clients under the epoch rule, is the row the second returns; routes and
    new_routes agree; sender, listener, ingress and route rows are ForwarderModel's.  Forged and replayed arrivals, which only the
    protected hop is sent, are dropped at its ingress and counted there and as malformed"""
    from hilcodec_amd.graph_step import GraphedForwardHop
    B, tb = B_HOP, wire.transport_bytes(N, M, T)
    sp = audio_level.SpeakerConfig(floor_level=50, margin_db=3) if speakers else None
    dl = downlink.DownlinkConfig(rate=rate.RateConfig(min_kbps=9.0, max_kbps=24.0)) if rated else None
    kw = dict(fec_stages=M, cng_order=K, cfg=CFG, max_arrivals=4 * B, downlink=dl, speakers=sp)
    hop = GraphedForwardHop(B, T, N, DEV, srtp=srtp.SrtpConfig(), **kw)
    ref = GraphedForwardHop(B, T, N, DEV, **kw)
    assert hop.wstride == wire.srtp_bytes(N, M, T) == tb + 10 and ref.wstride == ref.tstride == hop.tstride == tb
    assert "rekey_up" not in ref.stage.row and ref.arrivals.shape == hop.arrivals.shape
    model = forward_srtp.ForwarderModel(B, CFG, N, T, M, K, downlink=dl, speakers=sp)
    call = Call(B, N, T, M, K, seed=41 + speakers + 2 * rated, first={1: 0xFFF4, 6: 0xFFFA}, late=(2, 4, 9, 15))
    clients = Clients(B, CFG.fanout, tb)
    members, members_ref = Membership(B, N), Membership(B, N)

    def events(evs):
        members.apply(evs, hop)
        members_ref.apply(evs, ref)

    def uplink(b):
        mk, ms, ssrc = call.rekey(b)
        for keyed in (hop, model.keys):
            keyed.set_uplink_key(b, mk, ms, ssrc=ssrc)

    def downlink_key(b, tag, base):
        for keyed in (hop, model.keys):
            keyed.set_downlink_key(b, *key(tag, b), ssrc=base)
        clients.set_key(b, *key(tag, b), base)

    events([("join", b, b // 4) for b in range(B)])
    for b in range(B):
        uplink(b)
        if b != 7:                                           # listener 7 gets its key late: until then it is sent nothing
            downlink_key(b, 700, 31 * b)
    rng = np.random.default_rng(5)
    rejected = np.zeros(B, dtype=np.int64)
    for h in range(40):
        if h == 9:
            downlink_key(7, 700, 31 * 7)
        if h == 14:
            events([("join", 5, 0), ("layers", 0, 2), ("leave", 10)])
        if h == 22:
            uplink(13)                                       # a sender starts again under a new key
            downlink_key(3, 701, 12)
        if h == 30:
            events([("join", 10, 2)])
        plain, wired = call.hop()
        levels = rng.integers(0, 128, len(wired)).tolist() if speakers else None
        ref_levels = levels
        if h in (11, 19, 25) and wired:
            # in front of the hop's own arrivals: a forgery of one of them and, where there is one, its sender's arrival of three hops
            # ago once more; each carries the genuine arrival's level, so the slot's loudest level is what the plain hop sees
            again = [i for i, a in enumerate(wired) if any(o[0] == a[0] for o in call.history[h - 3])]
            i = again[0] if again else 0
            b, p = wired[i]
            bad = [(b, forge(p, 24 + int(rng.integers(0, 8 * (len(p) - 13)))))] + [o for o in call.history[h - 3] if o[0] == b][:1]
            wired = bad + wired
            levels = None if levels is None else [levels[i]] * len(bad) + levels
            rejected[b] += len(bad)
        reports = ([0, 5, 9], [0, 1, 0], [wire.pack_report(h & 255, 45 if h > 20 else 0, 0)] * 3) if rated and h % 4 == 3 else None
        fb = dict(reports=reports) if rated else {}
        slots, packets, nbytes = arrival_arrays(wired, tb + 10)
        out, out_nb = hop.forward(slots, torch.from_numpy(packets) if h % 2 else torch.from_numpy(packets).to(DEV), nbytes, levels, **fb)
        r_slots, r_packets, r_nbytes = arrival_arrays(plain, tb)
        ref_out, ref_nb = ref.forward(r_slots, torch.from_numpy(r_packets), r_nbytes, ref_levels, **fb)
        action = members.action()
        members_ref.action()
        want = model.step(slots, packets, nbytes, members.room, members.layers, action, levels=levels, reports=reports)
        out, out_nb = out.cpu().numpy(), out_nb.cpu().numpy()
        assert out.shape == (B, CFG.fanout, CFG.burst, tb + 10)
        assert np.array_equal(out_nb, want["out_nbytes"]) and np.array_equal(out, want["out"]), h
        epochs = hop.route_epoch.cpu().numpy()
        assert np.array_equal(hop.egress_state.cpu().numpy(), model.egress.state), h
        assert np.array_equal(hop.ingress_state.cpu().numpy(), model.ingress.state), h
        assert np.array_equal(hop.sender_state.cpu().numpy(), model.sender.state), h
        assert np.array_equal(hop.listener_state.cpu().numpy(), model.listener.state), h
        assert torch.equal(hop.routes, ref.routes) and torch.equal(hop.new_routes, ref.new_routes), h
        rows, counts = clients.deliver(epochs, out, out_nb)
        want_nb = ref_nb.cpu().numpy().copy()
        if h < 9:
            want_nb[7] = 0                                   # no key yet: plaintext never leaves
        assert np.array_equal(counts, want_nb), h
        assert np.array_equal(rows[want_nb > 0], ref_out.cpu().numpy()[want_nb > 0]), h
        if rated:
            assert torch.equal(hop.downlink_state, ref.downlink_state) and torch.equal(hop.eff_layers, ref.eff_layers), h
    rx, sd = hop.ingress_state.cpu().numpy(), hop.sender_state.cpu().numpy()
    assert rejected.sum() >= 4 and np.array_equal(rx[:, srtp.RX_AUTH_FAIL] + rx[:, srtp.RX_REPLAY], rejected)
    assert rx[:, srtp.RX_AUTH_FAIL].sum() >= 3 and rx[:, srtp.RX_REPLAY].sum() >= 1
    sd_ref = ref.sender_state.cpu().numpy().copy()
    sd_ref[:, forward.SD_MALFORMED] += rejected.astype(np.int32)
    assert np.array_equal(sd, sd_ref)
    eg = hop.egress_state.cpu().numpy()
    assert clients.delivered == eg[:, :, RT_PROTECTED].sum() > 300 and eg[7, :, RT_NOKEY].sum() > 0 and not eg[:, :, RT_STALE:].any()
    assert rx[1, srtp.RX_ROC] == 1 and eg[3, :, RT_EPOCH].min() >= 2


def test_views_keys_widths_and_reset():
    from hilcodec_amd.graph_step import GraphedForwardHop
    B, tb = 4, wire.transport_bytes(N, M, T)
    plain = GraphedForwardHop(B, T, N, DEV, fec_stages=M, cfg=CFG)
    for call in (lambda: plain.route_epoch, lambda: plain.egress_state, lambda: plain.ingress_state, lambda: plain.clear_keys(0),
                 lambda: plain.set_uplink_key(0, bytes(16), bytes(14)), lambda: plain.set_downlink_key(0, bytes(16), bytes(14))):
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(ValueError, match="history"):
        GraphedForwardHop(B, T, N, DEV, fec_stages=M, cfg=CFG, downlink=downlink.DownlinkConfig(history=8), srtp=srtp.SrtpConfig())
    hop = GraphedForwardHop(B, T, N, DEV, fec_stages=M, cfg=CFG, srtp=srtp.SrtpConfig())
    assert hop.route_epoch.shape == (B, 2) and hop.egress_state.shape == (B, 2, forward_srtp.RT_WORDS)
    assert hop.ingress_state.shape == (B, srtp.RX_WORDS)
    with pytest.raises(ValueError):                          # a plain packet's width
        hop.forward([0], torch.zeros(1, tb, dtype=torch.uint8), [tb])
    with pytest.raises(ValueError):
        hop.set_uplink_key(0, bytes(15), bytes(14))
    with pytest.raises(IndexError):
        hop.set_downlink_key(B, bytes(16), bytes(14))
    call = Call(B, N, T, M, None, seed=3)
    for b in range(B):
        hop.join(b, 0)
        mk, ms, ssrc = call.rekey(b)
        hop.set_uplink_key(b, mk, ms, ssrc=ssrc)
        hop.set_downlink_key(b, *key(800, b))
    for _ in range(3):
        _, wired = call.hop(p_flip=0.0)
        out, out_nb = hop.forward(*[torch.from_numpy(v) if isinstance(v, np.ndarray) else v for v in arrival_arrays(wired, tb + 10)])
    assert out_nb.any() and hop.egress_state[:, :, RT_PROTECTED].sum() >= (out_nb > 0).sum() > 0
    assert (hop.route_epoch == 1).all()
    hop.clear_keys(2)
    _, wired = call.hop(p_flip=0.0)
    out, out_nb = hop.forward(*[torch.from_numpy(v) if isinstance(v, np.ndarray) else v for v in arrival_arrays(wired, tb + 10)])
    assert not out_nb[2].any() and hop.egress_state[2, :, RT_NOKEY].any() and hop.ingress_state[2, srtp.RX_NOKEY] >= 1
    hop.reset()
    assert not hop.egress_state.any() and not hop.ingress_state.any() and hop.rooms == (-1,) * B and (hop.routes == -1).all()
    out, out_nb = hop.forward(*[torch.from_numpy(v) if isinstance(v, np.ndarray) else v for v in arrival_arrays(wired, tb + 10)])
    assert not out_nb.any() and not out.any() and hop.ingress_state[:, srtp.RX_NOKEY].sum() == len(wired)
    hop.set_uplink_key(0, *key(1, 0), ssrc=1000)             # reset forgot the old keys
