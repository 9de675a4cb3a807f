"""GPU: the selective forwarding hop (graph_step.GraphedForwardHop).  hilc_forward_classify and hilc_forward_route against forward.py's
models under tests/forward_loop.py's traffic; the graphed hop against the two ops called eagerly and against ForwardModel; the
forwarder behind a real sender, against reference senders at each listener's layers, and in front of a real receiver; the argument
checks.  Everything is integer: every comparison is bit for bit (torch.equal / np.array_equal)."""
import numpy as np
import pytest
import torch

from hilcodec_amd import forward, jitter, synth, wire
from hilcodec_amd.forward import ForwardConfig, ForwardModel, trim_packet
from hilcodec_amd.jitter import JitterConfig
from tests.forward_loop import Membership, Traffic, random_packet

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
HOP = 320
INTS = dict(dtype=torch.int32, device=DEV)


@pytest.fixture(scope="module")
def speech():
    return synth.streaming_model()


def dev(a, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).to(DEV)


class Rows:
    """the device rows of the two launches for B slots, filled so that an element a launch does not write shows"""

    def __init__(self, B, cfg, tb):
        F, P = cfg.fanout, cfg.burst
        self.sd, self.lr = torch.zeros(B, forward.SD_WORDS, **INTS), torch.zeros(B, forward.LR_WORDS, **INTS)
        self.pick, self.pick_count = torch.zeros(B, P, **INTS), torch.zeros(B, **INTS)
        self.routes, self.new_routes = torch.full((B, F), -1, **INTS), torch.zeros(B, F, **INTS)
        self.out, self.out_nbytes = torch.zeros(B, F, P, tb, dtype=torch.uint8, device=DEV), torch.zeros(B, F, P, **INTS)

    def spoil(self):
        for t in (self.pick, self.pick_count, self.new_routes, self.out_nbytes):
            t.fill_(-9)
        self.out.fill_(0xEE)

    def run(self, arr, offs, action, room, layers, cfg, n, T, m, K):
        from hilcodec_amd import ops
        self.spoil()
        ops.forward_classify(arr, offs, self.sd, self.pick, self.pick_count, cfg, n, T, m, K, action=action)
        ops.forward_route(arr, room, layers, self.sd, self.pick, self.pick_count, self.routes, self.new_routes, self.lr, self.out,
                          self.out_nbytes, cfg, n, T, m, K, action=action)

    def differs_from(self, res, model):
        """None, or the name of the first row that is not the model's"""
        got = dict(pick=self.pick, pick_count=self.pick_count, routes=self.routes, new_routes=self.new_routes, out=self.out,
                   out_nbytes=self.out_nbytes)
        for name, t in got.items():
            if not np.array_equal(t.cpu().numpy(), res[name]):
                return name
        if not np.array_equal(self.sd.cpu().numpy(), model.sender.state):
            return "sender_state"
        if not np.array_equal(self.lr.cpu().numpy(), model.listener.state):
            return "listener_state"
        return None


# (B, rooms): the ragged last workgroup of 4 waves; one room whose candidate scan goes past 64 lanes, with ties; nobody to route
NMK = [(8, 0, None), (8, 2, 8)]
FP = [(1, 1), (3, 2), (8, 4)]
KERNEL_CASES = [(5, 2, T, nmk, fp, keep) for T in (1, 3) for nmk in NMK for fp in FP for keep in (False, True)]
KERNEL_CASES += [(70, 1, 1, NMK[0], FP[2], True), (70, 1, 3, NMK[1], FP[1], False), (70, 1, 1, NMK[1], FP[0], True)]
KERNEL_CASES += [(1, 1, 1, NMK[0], FP[1], True), (1, 1, 3, NMK[1], FP[2], False)]


@pytest.mark.parametrize("case", KERNEL_CASES, ids=lambda c: "B{}-rooms{}-T{}-n{}m{}K{}-F{}P{}-fec{}".format(c[0], c[1], c[2], *c[3], *c[4], int(c[5])))
def test_kernels_against_the_model(case):
    """64 hops of the generator's traffic with joins, leaves and layer changes: every row, output byte, byte count, route, flag and
    counter of both launches is the model's on every hop"""
    B, rooms, T, (n, m, K), (F, P), keep_fec = case
    cfg = ForwardConfig(fanout=F, burst=P, hang_hops=3, keep_fec=keep_fec)
    model, mem = ForwardModel(B, cfg, n, T, m, K), Membership(B, n)
    net = Traffic(B, n, T, m, K, rooms, seed=B + 7 * T + m + F, p_event=0.3)
    tb = model.tb
    assert (tb == 13) == (m == 0 and T == 1)                 # 13: no multiple of 4
    rows = Rows(B, cfg, tb)
    mem.apply(net.initial_events())
    forwarded = 0
    for h in range(64):
        mem.apply(net.events())
        slots, packets, nbytes = net.hop()
        rec, offs = forward.arrival_records(slots, packets, nbytes, tb, B, 8 * B)
        assert len(slots) <= 8 * B
        action = mem.action()
        want = model.step_records(rec, offs, action, mem.room, mem.layers)
        rows.run(dev(rec), dev(offs), dev(action), dev(mem.room), dev(mem.layers), cfg, n, T, m, K)
        assert rows.differs_from(want, model) is None, (h, rows.differs_from(want, model))
        forwarded += int((want["out_nbytes"] > 0).sum())
    sd, lr = model.sender.state, model.listener.state
    if B > 1:                                                # the traffic reached every counter
        assert all(sd[:, i].sum() > 0 for i in range(forward.SD_WORDS) if i != forward.SD_SIDS or K is not None), sd.sum(axis=0)
        assert forwarded > 0 and lr[:, forward.LR_TRIMMED].sum() > 0 and lr[:, forward.LR_SWITCHES].sum() > 0
    else:
        assert forwarded == 0 and not lr.any()
    # without an action row no slot is cleared
    want = model.step_records(rec, offs, np.zeros(B, dtype=np.int32), mem.room, mem.layers)
    rows.run(dev(rec), dev(offs), None, dev(mem.room), dev(mem.layers), cfg, n, T, m, K)
    assert rows.differs_from(want, model) is None


def test_layers_below_m_drop_the_fec_flag():
    """a listener with layers = 1 and m = 2: rows without the FEC flag, wire.fec_primary of the one-stage cut behind the rewritten
    header, as trim_packet says"""
    B, n, T, m = 2, 8, 3, 2
    cfg = ForwardConfig(fanout=1, burst=1)
    rng = np.random.default_rng(5)
    packet, codes = random_packet(rng, 4321, 6, T, m, True)
    tb = wire.transport_bytes(n, m, T)
    rec, offs = forward.arrival_records([1], np.frombuffer(packet.ljust(tb, b"\0"), dtype=np.uint8)[None], [len(packet)], tb, B, 4)
    rows = Rows(B, cfg, tb)
    rows.run(dev(rec), dev(offs), dev([1, 1]), dev([0, 0]), dev([1, 8]), cfg, n, T, m, None)
    nb = int(rows.out_nbytes[0, 0, 0])
    got = bytes(rows.out[0, 0, 0, :nb].tolist())
    want = wire.pack_transport(4321, wire.fec_primary(packet[3:], 1, T), 1, fec=False)
    assert got == want == trim_packet(packet, len(packet), 1, T, n, m, None, True) and nb == 3 + wire.packet_bytes(1, T)
    assert not got[2] & wire.FEC_BIT and not rows.out[0, 0, 0, nb:].any()
    assert rows.routes.tolist() == [[1], [-1]] and rows.lr[0].tolist() == [1, nb, 1, 1]


# ---------------------------------------------------------------- the graphed hop
def test_graph_against_eager_and_model():
    """GraphedForwardHop.forward over 40 hops (some without arrivals, most without a session change) equals the two ops called eagerly
    on the same staged inputs and ForwardModel; what it returned stays valid for one further call"""
    from hilcodec_amd.graph_step import GraphedForwardHop
    B, n, T, m, K = 9, 8, 1, 2, 8
    cfg = ForwardConfig(fanout=3, burst=2, hang_hops=3)
    hop = GraphedForwardHop(B, T, n, DEV, fec_stages=m, cng_order=K, cfg=cfg, max_arrivals=8 * B)
    model, mem = ForwardModel(B, cfg, n, T, m, K), Membership(B, n)
    net = Traffic(B, n, T, m, K, 2, seed=31, p_event=0.15)
    tb = model.tb
    assert hop.tstride == tb and hop.rooms == (-1,) * B and hop.layers == (n,) * B
    eager = Rows(B, cfg, tb)
    mem.apply(net.initial_events(), hop)
    held, quiet_hops, calm_hops = None, 0, 0
    for h in range(40):
        events = net.events() if h % 3 == 0 else []
        mem.apply(events, hop)
        slots, packets, nbytes = net.hop() if h % 7 != 5 else ([], np.zeros((0, tb), dtype=np.uint8), [])
        quiet_hops += not slots
        calm_hops += not events
        on_device = h % 2 == 1
        t_packets = torch.from_numpy(packets).to(DEV) if on_device else torch.from_numpy(packets)
        out, out_nbytes = hop.forward(slots, t_packets, nbytes)
        action = mem.action()
        want = model.step(slots, packets, nbytes, mem.room, mem.layers, action)
        assert hop.rooms == tuple(mem.room.tolist()) and hop.layers == tuple(mem.layers.tolist())
        st = hop.stage
        assert np.array_equal(st.row["action"].cpu().numpy(), action) and np.array_equal(st.row["room"].cpu().numpy(), mem.room)
        eager.run(hop.arrivals.clone(), hop.offsets.clone(), st.row["action"].clone(), st.row["room"].clone(), st.row["layers"].clone(),
                  cfg, n, T, m, K)
        assert eager.differs_from(want, model) is None, (h, eager.differs_from(want, model))
        for name, t in (("out", out), ("out_nbytes", out_nbytes), ("routes", hop.routes), ("new_routes", hop.new_routes)):
            assert np.array_equal(t.cpu().numpy(), want[name]), (h, name)
        assert torch.equal(hop.sender_state, eager.sd) and torch.equal(hop.listener_state, eager.lr), h
        if held is not None:                                 # the previous call's views are still that call's result
            assert np.array_equal(held[0].cpu().numpy(), held[2]["out"]) and np.array_equal(held[1].cpu().numpy(), held[2]["out_nbytes"]), h
        held = (out, out_nbytes, want)
    assert quiet_hops >= 3 and calm_hops >= 20 and model.listener.state[:, forward.LR_PACKETS].sum() > 50
    with pytest.raises(ValueError):
        hop.forward([0] * (8 * B + 1), torch.zeros(8 * B + 1, tb, dtype=torch.uint8), [0] * (8 * B + 1))
    with pytest.raises(ValueError):
        hop.forward([0], torch.zeros(1, tb + 1, dtype=torch.uint8), [5])
    with pytest.raises(ValueError):
        hop.forward(torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(1, tb, dtype=torch.uint8), [5])
    with pytest.raises(IndexError):
        hop.forward([B], torch.zeros(1, tb, dtype=torch.uint8), [5])
    for bad in (lambda: hop.join(B, 0), lambda: hop.leave(-1), lambda: hop.set_layers(B, 1)):
        with pytest.raises(IndexError):
            bad()
    for bad in (lambda: hop.join(0, B), lambda: hop.join(0, -1), lambda: hop.set_layers(0, 0), lambda: hop.set_layers(0, n + 1),
                lambda: GraphedForwardHop(B, T, n, DEV, cfg=3), lambda: GraphedForwardHop(B, T, 32, DEV),
                lambda: GraphedForwardHop(B, T, n, DEV, fec_stages=n + 1)):
        with pytest.raises(ValueError):
            bad()


def test_against_a_real_sender_and_into_a_real_receiver(speech):
    """A sender of 4 slots at n = 8 with FEC and headers, forwarded in one room to listeners with layers (2, 3, 5, 8): every forwarded
    row equals the packet a reference sender at that n makes of the same clip (the quantiser is greedy: the first L stages and the
    redundant section do not depend on n), and the sender's own packet at 8.  Listener 0's rows then play in a jitter receiver."""
    from hilcodec_amd.graph_step import GraphedDecodeHop, GraphedEncodeHop, GraphedForwardHop
    n, m, hops = 8, 2, 12
    LAYERS = (2, 3, 5, 8)
    kw = dict(sessions=True, fec_stages=m, header=True)
    tx = GraphedEncodeHop(speech, 4, HOP, n, DEV, **kw)
    ref = GraphedEncodeHop(speech, 12, HOP, n, DEV, **kw)
    for g, L in enumerate(LAYERS[:3]):
        for i in range(4):
            ref.set_bitrate(4 * g + i, L)
    fwd = GraphedForwardHop(4, 1, n, DEV, fec_stages=m, cfg=ForwardConfig(fanout=3))
    for b in range(4):
        fwd.join(b, 0)
        fwd.set_layers(b, LAYERS[b])
    rx = GraphedDecodeHop(speech, 3, 1, n, DEV, sessions=True, conceal=True, fec_stages=m, cng_order=None,
                          jitter=JitterConfig(depth=2, capacity=8))
    x = synth.synth_clips(4, HOP * hops, seed=14).to(DEV)
    tb = wire.transport_bytes(n, m, 1)
    played = with_fec = 0
    for h in range(hops):
        xs = x[:, :, HOP * h:HOP * (h + 1)].contiguous()
        packets, nbytes = tx.step(xs)
        r_packets, r_nbytes = ref.step(xs.repeat(3, 1, 1))
        sent, sent_nb = packets.cpu().numpy(), nbytes.cpu().numpy()
        want, want_nb = r_packets.cpu().numpy(), r_nbytes.cpu().numpy()
        assert (sent_nb == tb if h else sent_nb == 3 + wire.packet_bytes(n, 1)).all()
        out, out_nbytes = fwd.forward(list(range(4)), packets, sent_nb.tolist())
        got, got_nb, routes = out.cpu().numpy(), out_nbytes.cpu().numpy(), fwd.routes.cpu().numpy()
        for b, L in enumerate(LAYERS):
            assert sorted(routes[b].tolist()) == [t for t in range(4) if t != b], (h, b)
            for j in range(3):
                t = int(routes[b, j])
                row, nb = (want[4 * LAYERS.index(L) + t], want_nb[4 * LAYERS.index(L) + t]) if L < n else (sent[t], sent_nb[t])
                assert got_nb[b, j, 0] == nb and got_nb[b, j, 1] == 0, (h, b, j)
                assert np.array_equal(got[b, j, 0], row) and not got[b, j, 1].any(), (h, b, j)
                with_fec += int(bool(row[2] & wire.FEC_BIT))
        new = fwd.new_routes.cpu().numpy()
        assert new[0].all() == (h == 0) and new.any() == (h == 0)
        for j in np.nonzero(new[0])[0]:
            rx.start(int(j))
        rx.play([0, 1, 2], out[0, :, 0].contiguous(), got_nb[0, :, 0].tolist())
        played += int((got_nb[0] > 0).sum())
    js = rx.jitter_state.cpu().numpy()
    assert played == 3 * hops and with_fec == 12 * (hops - 1)
    assert js[:, jitter.STAT_MALFORMED].sum() == 0 and js[:, jitter.STAT_ACCEPTED].sum() == played
    assert fwd.listener_state.cpu().numpy()[:, forward.LR_TRIMMED].tolist() == [3 * hops] * 3 + [0]


# ---------------------------------------------------------------- argument checks
def test_argument_checks():
    """every bad argument returns its error code and launches nothing; the ops check the widths of their rows"""
    from hilcodec_amd import _lib, ops
    lib = _lib.lib
    SHAPE, NULL, RANGE = -1, -2, -5
    B, n, T, m, F, P, A = 3, 8, 1, 2, 3, 2, 6
    tb = wire.transport_bytes(n, m, T)
    aw = 1 + (tb + 3) // 4
    z = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt, device=DEV)
    arr, offs, act = z(A, aw), z(B + 1), z(B)
    r = Rows(B, ForwardConfig(fanout=F, burst=P), tb)
    room, layers = z(B), torch.full((B,), n, **INTS)
    p = lambda t: t.data_ptr()
    r.spoil()
    good = [p(arr), p(offs), A, p(act), p(r.sd), p(r.pick), p(r.pick_count), B, T, n, m, 8, P, 3, None]
    for i in (0, 1, 4, 5, 6):
        assert lib.hilc_forward_classify(*[None if j == i else v for j, v in enumerate(good)]) == NULL, i
    for i, v, code in ((2, -1, SHAPE), (7, 0, SHAPE), (8, 0, SHAPE), (8, 4000, SHAPE), (9, 0, RANGE), (9, 32, RANGE), (10, -1, RANGE),
                       (10, 9, RANGE), (9, 31, RANGE), (11, -2, RANGE), (11, 17, RANGE), (12, 0, RANGE), (12, 5, RANGE), (13, -1, RANGE),
                       (13, 256, RANGE)):
        assert lib.hilc_forward_classify(*[v if j == i else w for j, w in enumerate(good)]) == code, (i, v)
    good2 = [p(arr), A, p(act), p(room), p(layers), p(r.sd), p(r.pick), p(r.pick_count), p(r.routes), p(r.new_routes), p(r.lr), p(r.out),
             p(r.out_nbytes), B, T, n, m, 8, F, P, 1, None]
    for i in (0, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12):
        assert lib.hilc_forward_route(*[None if j == i else v for j, v in enumerate(good2)]) == NULL, i
    for i, v, code in ((1, -1, SHAPE), (13, 0, SHAPE), (14, 0, SHAPE), (14, 4000, SHAPE), (15, 0, RANGE), (15, 32, RANGE), (16, -1, RANGE),
                       (16, 9, RANGE), (17, -2, RANGE), (17, 17, RANGE), (18, 0, RANGE), (18, 9, RANGE), (19, 0, RANGE), (19, 5, RANGE)):
        assert lib.hilc_forward_route(*[v if j == i else w for j, w in enumerate(good2)]) == code, (i, v)
    torch.cuda.synchronize()
    assert bool((r.out == 0xEE).all()) and all(bool((t == -9).all()) for t in (r.pick, r.pick_count, r.new_routes, r.out_nbytes))
    assert not r.sd.any() and not r.lr.any() and bool((r.routes == -1).all())      # a refused call launches nothing
    assert lib.hilc_forward_classify(*good) == 0 and lib.hilc_forward_route(*good2) == 0
    assert lib.hilc_forward_classify(*[None if j == 3 else v for j, v in enumerate(good)]) == 0      # the action row is optional
    assert lib.hilc_forward_route(*[None if j == 2 else v for j, v in enumerate(good2)]) == 0
    torch.cuda.synchronize()
    assert not r.out.any() and not r.out_nbytes.any() and bool((r.pick == -1).all()) and not r.pick_count.any()
    cfg = ForwardConfig(fanout=F, burst=P)
    c_args = dict(arrivals=arr, offsets=offs, rows=r.sd, pick=r.pick, pick_count=r.pick_count)
    for name, bad in (("arrivals", z(A, aw + 1)), ("offsets", z(B)), ("rows", z(B, forward.SD_WORDS + 1)), ("pick", z(B, P + 1))):
        with pytest.raises(RuntimeError):
            ops.forward_classify(**{**c_args, name: bad}, cfg=cfg, n=n, frames=T, m=m)
    r_args = dict(arrivals=arr, room=room, layers=layers, sender_rows=r.sd, pick=r.pick, pick_count=r.pick_count, routes=r.routes,
                  new_routes=r.new_routes, rows=r.lr, out=r.out, out_nbytes=r.out_nbytes)
    for name, bad in (("arrivals", z(A, aw - 1)), ("layers", z(B + 1)), ("sender_rows", z(B, 5)), ("pick", z(B, P + 1)),
                      ("routes", z(B, F + 1)), ("new_routes", z(B + 1, F)), ("rows", z(B, 3)), ("out", z(B, F, P, tb + 1, dt=torch.uint8)),
                      ("out_nbytes", z(B, F, P + 1)), ("pick_count", z(B + 2))):
        with pytest.raises(RuntimeError):
            ops.forward_route(**{**r_args, name: bad}, cfg=cfg, n=n, frames=T, m=m)
    with pytest.raises(RuntimeError):
        ops.forward_route(**{**r_args, "out": r.out.cpu()}, cfg=cfg, n=n, frames=T, m=m)      # no CPU fallback
