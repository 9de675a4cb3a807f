"""GPU: the downlink control of the forwarding hop (graph_step.GraphedForwardHop(downlink=)).  hilc_downlink_store and
hilc_downlink_step against downlink.py's model under tests/downlink_loop.py's traffic and feedback; the graphed hop against the four ops
called eagerly and against the model; the hop without the option; a real sender in front of the forwarder and a real receiver with reports
and NACKs behind it; the argument checks.  Everything is integer: every comparison is bit for bit."""
import numpy as np
import pytest
import torch

from hilcodec_amd import downlink, forward, jitter, rtx, synth, wire
from hilcodec_amd.downlink import DownlinkConfig, ForwardDownlinkModel
from hilcodec_amd.forward import ForwardConfig, ForwardModel, trim_packet
from hilcodec_amd.jitter import JitterConfig
from hilcodec_amd.rate import RateConfig
from hilcodec_amd.report import ReportConfig
from hilcodec_amd.rtx import NackConfig
from tests.downlink_loop import Feedback, run_random
from tests.forward_loop import Membership, Traffic

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
HOP = 320
INTS = dict(dtype=torch.int32, device=DEV)


@pytest.fixture(scope="module")
def speech():
    return synth.streaming_model()


def dev(a, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).to(DEV)


def rate_for(T, m, fcfg, timeout_hops=10):
    """a RateConfig whose minimum just pays for the floor of a hop, so that the bucket limits some hops and not others"""
    floor = downlink.floor_bits(T, m, fcfg.fanout, fcfg.keep_fec)
    kbps = (floor + 1) * 24000.0 / (1000.0 * T * 320.0)
    return RateConfig(min_kbps=kbps, max_kbps=2 * kbps, start_kbps=kbps, burst_hops=3, timeout_hops=timeout_hops)


class Rows:
    """the device rows of the four launches for B slots; spoil() fills what a launch must write so that an element it misses shows"""

    def __init__(self, B, fcfg, dcfg, tb):
        F, P, R, Q = fcfg.fanout, fcfg.burst, dcfg.history, dcfg.per_hop
        z = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt, device=DEV)
        self.sd, self.lr, self.pick, self.pick_count = z(B, forward.SD_WORDS), z(B, forward.LR_WORDS), z(B, P), z(B)
        self.routes, self.new_routes = torch.full((B, F), -1, **INTS), z(B, F)
        self.route_out, self.route_nbytes = z(B, F, P, tb, dt=torch.uint8), z(B, F, P)
        self.dl, self.mem, self.eff = z(B, downlink.DL_WORDS), z(B, F), z(B)
        self.out, self.out_nbytes = z(B, F, P, tb, dt=torch.uint8), z(B, F, P)
        self.history = None
        if R:
            self.tags, self.ring, self.ds = z(B, R), z(B, R, 1 + (tb + 3) // 4), z(B, downlink.DS_WORDS)
            self.rtx, self.rtx_nbytes, self.rtx_routes = z(B, Q, tb, dt=torch.uint8), z(B, Q), z(B, Q)
            self.history = dict(tags=self.tags, ring=self.ring, rtx_out=self.rtx, rtx_nbytes=self.rtx_nbytes, rtx_routes=self.rtx_routes)

    def start(self, model):
        """the listener rows as the model has them after a reset (every slot is joined on the first hop anyway)"""
        self.dl.copy_(dev(model.downlink.state))

    def spoil(self):
        for t in (self.pick, self.pick_count, self.new_routes, self.route_nbytes, self.out_nbytes, self.eff):
            t.fill_(-9)
        self.route_out.fill_(0xEE)
        self.out.fill_(0xEE)
        if self.history:
            self.rtx.fill_(0xEE), self.rtx_nbytes.fill_(-9), self.rtx_routes.fill_(-9)

    def run(self, arr, offs, action, room, layers, fb, fcfg, dcfg, n, T, m, K):
        from hilcodec_amd import ops
        self.spoil()
        ops.forward_classify(arr, offs, self.sd, self.pick, self.pick_count, fcfg, n, T, m, K, action=action)
        ops.forward_route(arr, room, layers, self.sd, self.pick, self.pick_count, self.routes, self.new_routes, self.lr, self.route_out,
                          self.route_nbytes, fcfg, n, T, m, K, action=action)
        if self.history:
            ops.downlink_store(arr, self.pick, self.pick_count, self.tags, self.ring, self.ds, n, T, m, action=action)
        ops.downlink_step(self.routes, self.new_routes, self.route_out, self.route_nbytes, layers, self.dl, self.mem, self.eff, self.out,
                          self.out_nbytes, dcfg, fcfg, n, T, m, action=action, **fb, **(self.history or {}))

    def differs_from(self, res, model):
        """None, or the name of the first row that is not the model's: every output byte and count, every state and memory word, every
        tag and history byte"""
        d = model.downlink
        got = dict(pick=self.pick, pick_count=self.pick_count, routes=self.routes, new_routes=self.new_routes, route_out=self.route_out,
                   route_nbytes=self.route_nbytes, out=self.out, out_nbytes=self.out_nbytes, eff_layers=self.eff)
        want = dict(res, sd=model.forward.sender.state, lr=model.forward.listener.state, dl=d.state, mem=d.memory)
        got.update(sd=self.sd, lr=self.lr, dl=self.dl, mem=self.mem)
        if self.history:
            got.update(rtx_packets=self.rtx, rtx_nbytes=self.rtx_nbytes, rtx_routes=self.rtx_routes, tags=self.tags, ring=self.ring, ds=self.ds)
            want.update(tags=d.tags, ring=d.ring, ds=d.sender_state)
        for name, t in got.items():
            if not np.array_equal(t.cpu().numpy(), want[name]):
                return name
        return None


def feedback_dev(step, dcfg):
    fb = {}
    if dcfg.rate is not None:
        fb["report"] = dev(step["report"])
    if dcfg.history:
        fb.update(nack_base=dev(step["nack_base"]), nack_bitmap=dev(step["nack_bitmap"]))
    return fb


# (B, rooms, T, (n, m, K), (fanout, burst), R, per_hop, what is on): the ragged last workgroup of 4 waves in two rooms; one room whose
# scan passes 64 lanes; one slot.  tb = 13 at T = 1, m = 0 is no multiple of 4; (8, 4) is 32 cells, and nine slots in one room fill
# them (the rooms of two and three never overdraw a bucket whose minimum pays the floor of eight routes)
NMK = [(8, 0, None), (8, 2, 8), (8, 1, None)]
KERNEL_CASES = [
    (5, 2, 1, NMK[0], (1, 1), 2, 1, "both"), (5, 2, 1, NMK[1], (3, 2), 16, 4, "both"), (5, 2, 3, NMK[2], (8, 4), 2, 4, "both"),
    (5, 2, 3, NMK[1], (3, 2), 16, 1, "rate"), (5, 2, 1, NMK[2], (3, 2), 16, 1, "history"), (5, 2, 1, NMK[0], (8, 4), 16, 4, "both"),
    (5, 2, 3, NMK[0], (1, 1), 2, 1, "history"), (5, 2, 1, NMK[1], (8, 4), 2, 1, "rate"), (70, 1, 1, NMK[1], (3, 2), 16, 4, "both"),
    (1, 1, 1, NMK[0], (3, 2), 2, 1, "both"), (1, 1, 3, NMK[1], (8, 4), 16, 4, "rate"), (9, 1, 1, NMK[1], (8, 4), 16, 4, "both"),
]


@pytest.mark.parametrize("case", KERNEL_CASES, ids=lambda c: "B{}-rooms{}-T{}-n{}m{}K{}-F{}P{}-R{}Q{}-{}".format(c[0], c[1], c[2], *c[3], *c[4], *c[5:]))
def test_kernels_against_the_model(case):
    """64 hops of the generators' traffic and feedback with joins, leaves and layer changes: every state word, memory word, tag,
    history byte, output byte and count of the launches is the model's on every hop; the outputs are spoilt before each hop"""
    B, rooms, T, (n, m, K), (F, P), R, Q, on = case
    fcfg = ForwardConfig(fanout=F, burst=P, hang_hops=3, keep_fec=(B + T + F) % 2 == 0)
    dcfg = DownlinkConfig(rate=rate_for(T, m, fcfg) if on != "history" else None, history=R if on != "rate" else 0, per_hop=Q)
    shape = dict(B=B, n=n, T=T, m=m, K=K, rooms=rooms)
    steps, model = run_random(shape, fcfg, dcfg, 65, seed=B + 7 * T + m + F + R, p_event=0.15, feedback_kw=dict(p_report=0.3, p_nack=0.3))
    # the model ran ahead: a second one follows hop by hop, for the state after each hop
    follow = ForwardDownlinkModel(B, fcfg, dcfg, n, T, m, K)
    tb = follow.tb
    assert (tb == 13) == (m == 0 and T == 1)
    rows = Rows(B, fcfg, dcfg, tb)
    rows.start(follow)
    for h, st in enumerate(steps):
        max_a = max(8 * B, len(st["rec"]))
        rec = np.zeros((max_a, st["rec"].shape[1]), dtype=np.int32)
        rec[:len(st["rec"])] = st["rec"]
        last = h == len(steps) - 1                             # the last hop runs without an action row: no slot is cleared
        action = np.zeros(B, dtype=np.int32) if last else st["action"]
        fb = {k: st[k] for k in ("report", "nack_base", "nack_bitmap")}
        want = follow.step_records(st["rec"], st["offs"], action, st["room"], st["layers"], **fb)
        rows.run(dev(rec), dev(st["offs"]), None if last else dev(action), dev(st["room"]), dev(st["layers"]), feedback_dev(st, dcfg),
                 fcfg, dcfg, n, T, m, K)
        assert rows.differs_from(want, follow) is None, (h, rows.differs_from(want, follow))
    d = follow.downlink
    if B > 1:                                                  # the traffic reached the rules that are on
        names = ["packets", "bytes"]
        names += ["reports", "stale", "decreased", "increased"] * (dcfg.rate is not None)
        names += ["limited", "trimmed"] * (dcfg.rate is not None and (F < 8 or B >= 9))
        names += ["nack_stale", "requests", "rtx_sent", "rtx_miss"] * (dcfg.history > 0)
        counts = {k: int(d.state[:, downlink.DL_REPORTS + downlink.DL_NAMES.index(k)].sum()) for k in names}
        assert all(v > 0 for v in counts.values()), counts
        assert dcfg.history == 0 or d.sender_state[:, downlink.DS_STORED].sum() > 0
    else:
        assert not d.state[:, downlink.DL_PACKETS].any()


# ---------------------------------------------------------------- the graphed hop
def test_graph_against_eager_and_model():
    """GraphedForwardHop(downlink=).forward over 40 hops — some without arrivals, some without feedback, some with feedback on
    consecutive hops, which must apply to one hop each — equals the four ops called eagerly on the same staged inputs and the model;
    what it returned and its ping-pong views stay valid for one further call"""
    from hilcodec_amd.graph_step import GraphedForwardHop
    B, n, T, m, K = 9, 8, 1, 2, 8
    fcfg = ForwardConfig(fanout=3, burst=2, hang_hops=3)
    dcfg = DownlinkConfig(rate=rate_for(T, m, fcfg), history=8, per_hop=2)
    hop = GraphedForwardHop(B, T, n, DEV, fec_stages=m, cng_order=K, cfg=fcfg, max_arrivals=8 * B, downlink=dcfg)
    model, mem = ForwardDownlinkModel(B, fcfg, dcfg, n, T, m, K), Membership(B, n)
    net, fbk = Traffic(B, n, T, m, K, 2, seed=31, p_event=0.15), Feedback(B, fcfg.fanout, dcfg.history, 31, p_report=0.3, p_nack=0.3)
    tb = model.tb
    eager = Rows(B, fcfg, dcfg, tb)
    eager.start(model)
    assert np.array_equal(hop.downlink_state.cpu().numpy(), model.downlink.state) and bool((hop.eff_layers == n).all())
    mem.apply(net.initial_events(), hop)
    held, quiet_hops, no_feedback, consecutive, fed_before = None, 0, 0, 0, False
    VIEWS = ("eff_layers", "rtx_packets", "rtx_nbytes", "rtx_routes")
    for h in range(40):
        mem.apply(net.events() if h % 3 == 0 else [], hop)
        reports, nacks = fbk.hop(model.forward.listener.routes, net.h)
        if h % 5 in (3, 4):
            reports = nacks = None
        elif h % 5 == 2:
            nacks = None
        slots, packets, nbytes = net.hop() if h % 7 != 5 else ([], np.zeros((0, tb), dtype=np.uint8), [])
        quiet_hops += not slots
        no_feedback += reports is None and nacks is None
        consecutive += fed_before and reports is not None
        fed_before = reports is not None
        t_packets = torch.from_numpy(packets).to(DEV) if h % 2 else torch.from_numpy(packets)
        if h % 4 == 1 and reports is not None:                 # blobs as a uint8 tensor
            reports = (reports[0], torch.tensor(reports[1], dtype=torch.int64), torch.tensor([list(b) for b in reports[2]], dtype=torch.uint8).reshape(-1, 3))
        out, out_nbytes = hop.forward(slots, t_packets, nbytes, reports=reports, nacks=nacks)
        action = mem.action()
        want = model.step(slots, packets, nbytes, mem.room, mem.layers, action, reports=reports, nacks=nacks)
        rows = downlink.feedback_rows(B, fcfg.fanout, reports, nacks)
        st = hop.stage
        for name in ("report", "nack_base", "nack_bitmap"):    # exactly this hop's feedback is on the device
            assert np.array_equal(hop._fb[name].cpu().numpy(), rows[name]), (h, name)
        eager.run(hop.arrivals.clone(), hop.offsets.clone(), st.row["action"].clone(), st.row["room"].clone(), st.row["layers"].clone(),
                  {k: v.clone() for k, v in hop._fb.items()}, fcfg, dcfg, n, T, m, K)
        assert eager.differs_from(want, model) is None, (h, eager.differs_from(want, model))
        got = dict(out=out, out_nbytes=out_nbytes, routes=hop.routes, new_routes=hop.new_routes, **{v: getattr(hop, v) for v in VIEWS})
        for name, t in got.items():
            assert np.array_equal(t.cpu().numpy(), want[name]), (h, name)
        assert torch.equal(hop.downlink_state, eager.dl) and torch.equal(hop.history_state, eager.ds), h
        assert torch.equal(hop.sender_state, eager.sd) and torch.equal(hop.listener_state, eager.lr), h
        assert np.array_equal(downlink.kbps(hop.downlink_state, T), downlink.kbps(model.downlink.state, T))
        if held is not None:                                   # the previous call's views are still that call's result
            for name, t in held[0].items():
                assert np.array_equal(t.cpu().numpy(), held[1][name]), (h, name)
        held = ({k: got[k] for k in ("out", "out_nbytes") + VIEWS}, want)
    d = model.downlink.state
    assert quiet_hops >= 3 and no_feedback >= 12 and consecutive >= 8
    assert all(d[:, w].sum() > 0 for w in (downlink.DL_REPORTS, downlink.DL_RTX_SENT, downlink.DL_LIMITED, downlink.DL_PACKETS))
    # the argument errors, each checked before anything is uploaded
    good_r, good_n = wire.pack_report(1, 2, 3), wire.pack_nack(5, 0)
    empty = ([], torch.zeros(0, tb, dtype=torch.uint8), [])
    before = hop.downlink_state.clone()
    for kw in (dict(reports=([B], [0], [good_r])), dict(reports=([-1], [0], [good_r])), dict(reports=([0], [3], [good_r])),
               dict(nacks=([0], [-1], [good_n])), dict(nacks=([0], [0], [good_r])), dict(reports=([0], [0], [good_n])),
               dict(reports=([0, 1], [0], [good_r])), dict(reports=([0], [0])), dict(nacks=7),
               dict(reports=(torch.zeros(1, dtype=torch.int64, device=DEV), [0], [good_r])),
               dict(nacks=([0], [0], torch.zeros(1, 4, dtype=torch.uint8, device=DEV))),
               dict(reports=([0], [0], torch.zeros(1, 4, dtype=torch.uint8)))):
        with pytest.raises(ValueError):
            hop.forward(*empty, **kw)
    assert torch.equal(hop.downlink_state, before)             # nothing ran
    for bad in (dict(downlink=RateConfig(min_kbps=9.0, max_kbps=24.0)), dict(downlink=DownlinkConfig(rate=RateConfig(min_kbps=1.0, max_kbps=24.0)))):
        with pytest.raises(ValueError):
            GraphedForwardHop(B, T, n, DEV, cfg=fcfg, **bad)
    # one option without the other: the views and arguments of the missing one raise
    rate_only = GraphedForwardHop(3, T, n, DEV, cfg=fcfg, downlink=DownlinkConfig(rate=rate_for(T, 0, fcfg)))
    for bad in (lambda: rate_only.rtx_packets, lambda: rate_only.rtx_nbytes, lambda: rate_only.rtx_routes, lambda: rate_only.history_state,
                lambda: rate_only.forward([], torch.zeros(0, 13, dtype=torch.uint8), [], nacks=([0], [0], [good_n]))):
        with pytest.raises(RuntimeError):
            bad()
    history_only = GraphedForwardHop(3, T, n, DEV, cfg=fcfg, downlink=DownlinkConfig(history=4))
    with pytest.raises(RuntimeError):
        history_only.forward([], torch.zeros(0, 13, dtype=torch.uint8), [], reports=([0], [0], [good_r]))
    assert history_only.rtx_routes.shape == (3, 2) and bool((history_only.rtx_routes == -1).all()) and rate_only.eff_layers.shape == (3,)


def test_without_downlink_the_hop_is_unchanged():
    """GraphedForwardHop without downlink= returns ForwardModel's bytes, allocates none of the downlink state, and raises on
    reports=, nacks= and the downlink views"""
    from hilcodec_amd.graph_step import GraphedForwardHop
    B, n, T, m, K = 6, 8, 1, 2, 8
    fcfg = ForwardConfig(fanout=3, burst=2, hang_hops=3)
    hop = GraphedForwardHop(B, T, n, DEV, fec_stages=m, cng_order=K, cfg=fcfg, max_arrivals=8 * B)
    assert hop.downlink is None and not hasattr(hop, "_dl") and set(hop.stage.row) == {"action", "room", "layers"}
    model, mem, net = ForwardModel(B, fcfg, n, T, m, K), Membership(B, n), Traffic(B, n, T, m, K, 2, seed=5, p_event=0.2)
    mem.apply(net.initial_events(), hop)
    for h in range(20):
        mem.apply(net.events(), hop)
        slots, packets, nbytes = net.hop()
        out, out_nbytes = hop.forward(slots, torch.from_numpy(packets), nbytes)
        want = model.step(slots, packets, nbytes, mem.room, mem.layers, mem.action())
        assert np.array_equal(out.cpu().numpy(), want["out"]) and np.array_equal(out_nbytes.cpu().numpy(), want["out_nbytes"]), h
    assert model.listener.state[:, forward.LR_PACKETS].sum() > 20
    empty = ([], torch.zeros(0, hop.tstride, dtype=torch.uint8), [])
    for bad in (lambda: hop.forward(*empty, reports=([0], [0], [wire.pack_report(1, 2, 3)])), lambda: hop.forward(*empty, reports=([], [], [])),
                lambda: hop.forward(*empty, nacks=([0], [0], [wire.pack_nack(1, 0)])), lambda: hop.eff_layers, lambda: hop.downlink_state,
                lambda: hop.history_state, lambda: hop.rtx_packets, lambda: hop.rtx_nbytes, lambda: hop.rtx_routes):
        with pytest.raises(RuntimeError):
            bad()


# ---------------------------------------------------------------- real ends
def test_real_sender_forwarder_and_receiver(speech):
    """A 4-slot sender with headers and FEC feeds the forwarder with downlink=; listener 0's rows play in a 3-slot jitter receiver with
    reports and NACKs, whose feedback goes back where it is due.  A scripted set of forwarded rows is withheld: the retransmitted rows
    are trim_packet of the sender's original packet, the receiver counts them recovered, nothing is malformed, and every view of the
    forwarder equals the model run alongside"""
    from hilcodec_amd.graph_step import GraphedDecodeHop, GraphedEncodeHop, GraphedForwardHop
    n, m, hops, B = 8, 2, 40, 4
    fcfg = ForwardConfig(fanout=3, burst=2)
    nack = NackConfig(rtt_hops=2, retry_hops=3, max_requests=2)
    dcfg = DownlinkConfig(rate=RateConfig(min_kbps=9.0, max_kbps=36.0, burst_hops=4), history=16, per_hop=2)
    tx = GraphedEncodeHop(speech, B, HOP, n, DEV, sessions=True, fec_stages=m, header=True)
    fwd = GraphedForwardHop(B, 1, n, DEV, fec_stages=m, cfg=fcfg, downlink=dcfg)
    rx = GraphedDecodeHop(speech, 3, 1, n, DEV, sessions=True, conceal=True, fec_stages=m, cng_order=None,
                          jitter=JitterConfig(depth=4, capacity=8), report=ReportConfig(window=16, interval=8), nack=nack, max_arrivals=15)
    model = ForwardDownlinkModel(B, fcfg, dcfg, n, 1, m, None)
    for b in range(B):
        fwd.join(b, 0)
    room, layers = np.zeros(B, dtype=np.int32), np.full(B, n, dtype=np.int32)
    x = synth.synth_clips(B, HOP * hops, seed=14).to(DEV)
    tb = wire.transport_bytes(n, m, 1)
    # (hop, route) of listener 0: never two hops running on a route (the second would be asked for a hop later, and a retransmission
    # that arrives on the hop that plays it counts expired, not recovered)
    withheld = {(5, 0), (9, 1), (11, 1), (14, 2), (20, 0), (20, 2), (27, 1), (33, 0)}
    originals, nacks_due, reports_due, resent = {}, {}, [], 0
    for h in range(hops):
        packets, nbytes = tx.step(x[:, :, HOP * h:HOP * (h + 1)].contiguous())
        sent, sent_nb = packets.cpu().numpy(), nbytes.cpu().numpy()
        for t in range(B):
            originals[t, (int(sent[t, 0]) << 8) | int(sent[t, 1])] = sent[t, :sent_nb[t]].tobytes()
        due = nacks_due.pop(h, [])
        nk = ([0] * len(due), [j for j, _ in due], [blob for _, blob in due])
        rp = ([0] * len(reports_due), [j for j, _ in reports_due], [blob for _, blob in reports_due])
        out, out_nbytes = fwd.forward(list(range(B)), packets, sent_nb.tolist(), reports=rp, nacks=nk)
        want = model.step(list(range(B)), sent, sent_nb.tolist(), room, layers, np.full(B, int(h == 0), dtype=np.int32), reports=rp, nacks=nk)
        got = dict(out=out, out_nbytes=out_nbytes, routes=fwd.routes, new_routes=fwd.new_routes, eff_layers=fwd.eff_layers,
                   rtx_packets=fwd.rtx_packets, rtx_nbytes=fwd.rtx_nbytes, rtx_routes=fwd.rtx_routes)
        for name, t in got.items():
            assert np.array_equal(t.cpu().numpy(), want[name]), (h, name)
        d = model.downlink
        assert np.array_equal(fwd.downlink_state.cpu().numpy(), d.state) and np.array_equal(fwd.history_state.cpu().numpy(), d.sender_state), h
        eff = int(want["eff_layers"][0])
        arrived = []
        for j in range(3):
            if h == 0:
                rx.start(j)
            nb = int(want["out_nbytes"][0, j, 0])
            assert nb > 0 and want["out_nbytes"][0, j, 1] == 0
            if (h, j) not in withheld:
                arrived.append((j, want["out"][0, j, 0, :nb].tobytes()))
        for q in range(dcfg.per_hop):
            nb, j = int(want["rtx_nbytes"][0, q]), int(want["rtx_routes"][0, q])
            if nb:
                p = want["rtx_packets"][0, q, :nb].tobytes()
                orig = originals[int(want["routes"][0, j]), (p[0] << 8) | p[1]]
                assert p == trim_packet(orig, len(orig), eff, 1, n, m, None, True), (h, q)
                arrived.append((j, p))
                resent += 1
        rows = np.zeros((len(arrived), tb), dtype=np.uint8)
        for a, (_, p) in enumerate(arrived):
            rows[a, :len(p)] = np.frombuffer(p, dtype=np.uint8)
        rx.play([j for j, _ in arrived], torch.from_numpy(rows), [len(p) for _, p in arrived])
        ndue, nblobs = rx.nack_due.cpu().numpy(), rx.nacks.cpu().numpy()
        nacks_due[h + nack.rtt_hops] = [(j, nblobs[j].tobytes()) for j in range(3) if ndue[j]]
        rdue, rblobs = rx.report_due.cpu().numpy(), rx.reports.cpu().numpy()
        reports_due = [(j, rblobs[j].tobytes()) for j in range(3) if rdue[j]]
    js, nks = rx.jitter_state.cpu().numpy(), rx.nack_state.cpu().numpy()
    assert resent == len(withheld) == nks[:, rtx.NK_RECOVERED].sum() == model.downlink.state[0, downlink.DL_RTX_SENT]
    assert js[:, jitter.STAT_MALFORMED].sum() == 0 and js[:, jitter.STAT_LOST].sum() == 0
    assert model.downlink.state[0, downlink.DL_REPORTS] >= 9 and model.downlink.state[0, downlink.DL_RTX_MISS] == 0
    assert np.array_equal(model.forward.listener.routes[0], [1, 2, 3])


# ---------------------------------------------------------------- argument checks
def test_argument_checks():
    """every bad argument of both entry points returns its error code and launches nothing; the ops check the widths of their rows"""
    from hilcodec_amd import _lib, ops
    lib = _lib.lib
    SHAPE, NULL, RANGE = -1, -2, -5
    B, n, T, m, F, P, A, R, Q = 3, 8, 1, 2, 3, 2, 6, 4, 2
    fcfg = ForwardConfig(fanout=F, burst=P)
    dcfg = DownlinkConfig(rate=RateConfig(min_kbps=9.0, max_kbps=24.0), history=R, per_hop=Q)
    tb = wire.transport_bytes(n, m, T)
    aw = 1 + (tb + 3) // 4
    z = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt, device=DEV)
    arr, act, layers, fb = z(A, aw), z(B), torch.full((B,), n, **INTS), z(B, F)
    r = Rows(B, fcfg, dcfg, tb)
    r.pick.fill_(-1)
    p = lambda t: t.data_ptr()
    r.rtx.fill_(0xEE), r.out.fill_(0xEE), r.eff.fill_(-9), r.out_nbytes.fill_(-9)
    good = [p(arr), A, p(act), p(r.pick), p(r.pick_count), p(r.tags), p(r.ring), p(r.ds), B, T, n, m, P, R, None]
    for i in (0, 3, 4, 5, 6, 7):
        assert lib.hilc_downlink_store(*[None if j == i else v for j, v in enumerate(good)]) == NULL, i
    for i, v, code in ((1, -1, SHAPE), (8, 0, SHAPE), (9, 0, SHAPE), (9, 4000, SHAPE), (10, 0, RANGE), (10, 32, RANGE), (11, -1, RANGE),
                       (11, 9, RANGE), (12, 0, RANGE), (12, 5, RANGE), (13, 0, RANGE), (13, 1, RANGE), (13, 3, RANGE), (13, 128, RANGE)):
        assert lib.hilc_downlink_store(*[v if j == i else w for j, w in enumerate(good)]) == code, (i, v)
    good2 = [p(r.routes), p(r.new_routes), p(r.route_out), p(r.route_nbytes), p(layers), p(act), p(fb), p(fb), p(fb), p(r.tags), p(r.ring),
             p(r.dl), p(r.mem), p(r.eff), p(r.out), p(r.out_nbytes), p(r.rtx), p(r.rtx_nbytes), p(r.rtx_routes),
             B, T, n, m, F, P, 1, R, Q, 1, 120, 320, 320, 26, 5, 13, 8, 0, None]
    for i in (0, 1, 2, 3, 4, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 7, 8):      # 7, 8: one NACK row without the other
        assert lib.hilc_downlink_step(*[None if j == i else v for j, v in enumerate(good2)]) == NULL, i
    for i, v, code in ((19, 0, SHAPE), (20, 0, SHAPE), (20, 4000, SHAPE), (21, 0, RANGE), (21, 32, RANGE), (22, -1, RANGE), (22, 9, RANGE),
                       (23, 0, RANGE), (23, 9, RANGE), (24, 0, RANGE), (24, 5, RANGE), (26, 3, RANGE), (26, 128, RANGE), (26, 1, RANGE),
                       (27, 0, RANGE), (27, 5, RANGE), (29, 0, SHAPE), (29, 321, SHAPE), (30, 319, SHAPE), (30, (1 << 22) + 1, SHAPE),
                       (31, 119, SHAPE), (31, 321, SHAPE), (32, 256, RANGE), (32, 5, RANGE), (33, -1, RANGE), (34, -1, RANGE),
                       (34, 65536, RANGE), (35, 0, SHAPE), (35, 1 << 24, SHAPE), (36, -1, SHAPE)):
        assert lib.hilc_downlink_step(*[v if j == i else w for j, w in enumerate(good2)]) == code, (i, v)
    neither = [0 if j in (26, 28) else v for j, v in enumerate(good2)]
    assert lib.hilc_downlink_step(*neither) == RANGE                                   # neither rate nor history
    torch.cuda.synchronize()
    assert bool((r.out == 0xEE).all()) and bool((r.rtx == 0xEE).all()) and bool((r.eff == -9).all()) and bool((r.out_nbytes == -9).all())
    assert not r.dl.any() and not r.tags.any() and not r.ds.any() and not r.mem.any()      # a refused call launches nothing
    assert lib.hilc_downlink_store(*good) == 0 and lib.hilc_downlink_step(*good2) == 0
    assert lib.hilc_downlink_store(*[None if j == 2 else v for j, v in enumerate(good)]) == 0          # the action row is optional
    assert lib.hilc_downlink_step(*[None if j in (5, 6, 7, 8) else v for j, v in enumerate(good2)]) == 0        # and the feedback rows
    no_history = [None if j in (9, 10, 16, 17, 18) else (0 if j == 26 else v) for j, v in enumerate(good2)]
    assert lib.hilc_downlink_step(*no_history) == 0                                    # history 0: its rows are not read
    torch.cuda.synchronize()
    assert not r.out.any() and not r.out_nbytes.any() and bool((r.eff == n).all()) and not r.rtx.any() and bool((r.rtx_routes == -1).all())
    s_args = dict(arrivals=arr, pick=r.pick, pick_count=r.pick_count, tags=r.tags, ring=r.ring, rows=r.ds)
    for name, bad in (("arrivals", z(A, aw + 1)), ("pick", z(B + 1, P)), ("tags", z(B + 1, R)), ("ring", z(B, R, aw + 1)), ("ring", z(B, R + 1, aw)),
                      ("rows", z(B, downlink.DS_WORDS + 1)), ("tags", z(B, 3))):
        with pytest.raises((RuntimeError, AssertionError)):
            ops.downlink_store(**{**s_args, name: bad}, n=n, frames=T, m=m)
    with pytest.raises(RuntimeError):
        ops.downlink_store(**s_args, n=n, frames=T, m=m, action=z(B + 1))
    t_args = dict(routes=r.routes, new_routes=r.new_routes, packets=r.route_out, nbytes=r.route_nbytes, layers=layers, rows=r.dl, memory=r.mem,
                  eff_layers=r.eff, out=r.out, out_nbytes=r.out_nbytes, report=fb, nack_base=fb, nack_bitmap=fb, **r.history)
    for name, bad in (("routes", z(B, F + 1)), ("new_routes", z(B + 1, F)), ("packets", z(B, F, P, tb + 1, dt=torch.uint8)), ("nbytes", z(B, F, P + 1)),
                      ("layers", z(B + 1)), ("rows", z(B, downlink.DL_WORDS - 1)), ("memory", z(B, F + 1)), ("eff_layers", z(B + 1)),
                      ("out", z(B, F, P, tb - 1, dt=torch.uint8)), ("out_nbytes", z(B, F + 1, P)), ("report", z(B, F + 1)), ("nack_base", z(B + 1, F)),
                      ("nack_bitmap", z(B * F)), ("tags", z(B, 2 * R)), ("ring", z(B, R, aw - 1)), ("rtx_out", z(B, Q, tb + 1, dt=torch.uint8)),
                      ("rtx_out", z(B, Q + 1, tb, dt=torch.uint8)), ("rtx_nbytes", z(B, Q + 1)), ("rtx_routes", z(B + 1, Q)), ("tags", None),
                      ("rtx_routes", None)):
        with pytest.raises(RuntimeError):
            ops.downlink_step(**{**t_args, name: bad}, cfg=dcfg, fcfg=fcfg, n=n, frames=T, m=m)
    with pytest.raises(RuntimeError):
        ops.downlink_step(**{**t_args, "out": r.out.cpu()}, cfg=dcfg, fcfg=fcfg, n=n, frames=T, m=m)       # no CPU fallback
    with pytest.raises(RuntimeError):
        ops.downlink_store(**{**s_args, "ring": r.ring.cpu()}, n=n, frames=T, m=m)
    with pytest.raises(ValueError):                                                    # the floor of four routes is not paid for
        ops.downlink_step(**t_args, cfg=DownlinkConfig(rate=RateConfig(min_kbps=1.0, max_kbps=24.0), history=R, per_hop=Q), fcfg=fcfg, n=n, frames=T, m=m)
