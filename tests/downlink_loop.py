"""What the CPU and the GPU tests of the forwarding hop's downlink control share: a seeded feedback generator (report sequences that
progress, repeat and go back, losses across both thresholds, NACK bases inside, behind and ahead of the owner's history, feedback on free
and new routes), the run of the models under forward_loop.Traffic with it, and the two closed loops on the models alone (a bottleneck
shared by a listener's routes; iid downlink drops with NACK answers).  A plain module, imported as `from tests.downlink_loop import ...`."""
import numpy as np

from hilcodec_amd import downlink, forward, jitter, rtx, wire
from hilcodec_amd.downlink import DownlinkConfig, ForwardDownlinkModel
from hilcodec_amd.forward import ForwardConfig, ForwardModel
from hilcodec_amd.jitter import JitterConfig, JitterModel
from hilcodec_amd.rate import RateConfig
from hilcodec_amd.report import ReportModel
from hilcodec_amd.rtx import NackConfig, NackModel
from tests.forward_loop import Membership, Traffic
from tests.hops import arrival_arrays
from tests.rate_loop import LOOP_REPORT, Link, ReportLine


class Feedback:
    """seeded reports and NACKs for the B x fanout routes of a forwarding hop.  Per hop and route, whether it has an owner or not: with
    p_report a report whose seq mostly advances by one, sometimes repeats or goes back (stale), with a loss at or below `low`, between
    the thresholds or at and above `high`; with p_nack a NACK whose base lies inside the owner's history of R hops, behind it or ahead
    of what the owner has sent, with a sparse random bitmap.  `next_hop[t]`: the hop index sender t uses next (Traffic.h).  Each
    listener draws from a generator of its own, so one listener's feedback does not depend on another's."""

    def __init__(self, B, fanout, R, seed, p_report=0.25, p_nack=0.2, low=5, high=26, listener_seeds=None):
        self.B, self.F, self.R, self.low, self.high = B, fanout, max(R, 2), low, high
        self.rng = [np.random.default_rng([(listener_seeds or {}).get(b, seed), b, 77]) for b in range(B)]
        self.seq = np.zeros((B, fanout), dtype=np.int64)
        self.p_report, self.p_nack = p_report, p_nack

    def hop(self, routes, next_hop):
        """-> (reports, nacks), each (listeners, routes, blobs) as GraphedForwardHop.forward takes them; `routes` int [B, fanout]: the
        owners after the previous hop"""
        rep, nack = ([], [], []), ([], [], [])
        for b in range(self.B):
            rng = self.rng[b]
            for j in range(self.F):
                if rng.random() < self.p_report:
                    what = rng.random()
                    if what < 0.7:
                        self.seq[b, j] = (self.seq[b, j] + 1) & 255
                        seq = int(self.seq[b, j])
                    elif what < 0.85:
                        seq = int(self.seq[b, j])                         # repeated
                    else:
                        seq = int(self.seq[b, j] - rng.integers(1, 100)) & 255      # from before
                    kind = rng.random()
                    loss = int(rng.integers(0, self.low + 1)) if kind < 0.5 else \
                        int(rng.integers(self.low + 1, self.high)) if kind < 0.7 else int(rng.integers(self.high, 256))
                    rep[0].append(b), rep[1].append(j), rep[2].append(wire.pack_report(seq, loss, int(rng.integers(0, 256))))
                if rng.random() < self.p_nack:
                    t = int(routes[b, j])
                    newest = (int(next_hop[t]) - 1) if t >= 0 else int(rng.integers(0, 65536))
                    where = rng.random()
                    back = int(rng.integers(0, self.R)) if where < 0.6 else int(rng.integers(self.R, 3 * self.R)) if where < 0.8 \
                        else -int(rng.integers(1, 6))
                    bitmap = int(rng.integers(0, 65536)) & int(rng.integers(0, 65536)) & int(rng.integers(0, 65536))
                    nack[0].append(b), nack[1].append(j), nack[2].append(wire.pack_nack((newest - back) & 0xFFFF, bitmap))
        return rep, nack


def run_random(shape, fcfg, dcfg, hops, seed, p_event=0.2, feedback_kw=None, **traffic_kw):
    """ForwardDownlinkModel under Traffic and Feedback.  shape: dict(B, n, T, m, K, rooms).  Returns (per hop a dict: the staged inputs
    — rec, offs, action, room, layers, report, nack_base, nack_bitmap —, `res` everything the four launches write, and copies of the
    state after the hop: dl, mem, tags, ring, ds; the model)"""
    B, n, T, m, K, rooms = (shape[k] for k in ("B", "n", "T", "m", "K", "rooms"))
    net = Traffic(B, n, T, m, K, rooms, seed, p_event=p_event, **traffic_kw)
    fb = Feedback(B, fcfg.fanout, dcfg.history, seed, **(feedback_kw or {}))
    model, mem = ForwardDownlinkModel(B, fcfg, dcfg, n, T, m, K), Membership(B, n)
    mem.apply(net.initial_events())
    steps = []
    for _ in range(hops):
        mem.apply(net.events())
        reports, nacks = fb.hop(model.forward.listener.routes, net.h)
        slots, packets, nbytes = net.hop()
        rec, offs = forward.arrival_records(slots, packets, nbytes, model.tb, B)
        rows = downlink.feedback_rows(B, fcfg.fanout, reports if dcfg.rate is not None else None, nacks if dcfg.history else None)
        action = mem.action()
        res = model.step_records(rec, offs, action, mem.room, mem.layers, **rows)
        d = model.downlink
        steps.append(dict(rec=rec, offs=offs, action=action, room=mem.room.copy(), layers=mem.layers.copy(), res=res, dl=d.state.copy(),
                          mem=d.memory.copy(), tags=d.tags.copy(), ring=d.ring.copy(), ds=d.sender_state.copy(),
                          arrivals=(slots, packets, nbytes), reports=reports, nacks=nacks, **rows))
    return steps, model


# ---------------------------------------------------------------- the closed loops, on the models alone
N, T, FANOUT, SENDERS = 8, 1, 3, 4
LISTENER = SENDERS                                             # slot 4 listens and never talks; one room (Conference.listener)
LOOP_FORWARD = ForwardConfig(fanout=FANOUT, burst=2, hang_hops=8)
LOOP_RATE = RateConfig(min_kbps=9.0, max_kbps=24.0)            # binary-exact: 120 bits per hop (the floor of three routes) and 320
LOOP_JITTER = JitterConfig(depth=4, capacity=8)
LOOP_NACK = NackConfig(rtt_hops=2, retry_hops=3, max_requests=2)


class SharedLink(Link):
    """rate_loop.Link shared by the packets of one hop: drained once per hop, then offered each packet in turn (drop-tail)"""

    def hop_many(self, items):
        """items: [(key, bytes)] in offer order -> ([dropped per item], [(key, bytes) delivered on this hop])"""
        _, out = self.hop(b"")
        dropped = []
        for item in items:
            bits = 8 * len(item[1])
            self.sent += 1
            dropped.append(self.backlog + bits > 4 * self.cap)
            if dropped[-1]:
                self.dropped += 1
            else:
                self.queue.append([item, bits])
                self.backlog += bits
        return dropped, out


class Conference:
    """`senders` (four) always-talking senders (n = 8, T = 1, m = 0, random codes) and a silent listener in one room of a forwarder model, with
    `dcfg` (None: a ForwardModel alone) — the part the two closed loops share.  hop(t, ...) -> the rows for the listener as [(route,
    bytes)], route order, and the hop's result"""

    def __init__(self, dcfg, seed, uplink_loss=None, senders=SENDERS):
        self.senders, self.listener = senders, senders         # the slot behind the senders listens and never talks
        self.B, self.tb = senders + 1, wire.transport_bytes(N, 0, T)
        self.model = ForwardModel(self.B, LOOP_FORWARD, N, T) if dcfg is None else ForwardDownlinkModel(self.B, LOOP_FORWARD, dcfg, N, T)
        self.dcfg, self.rng, self.uplink_loss = dcfg, np.random.default_rng(seed), uplink_loss or {}
        self.room, self.layers = np.zeros(self.B, dtype=np.int32), np.full(self.B, N, dtype=np.int32)
        self.originals = {}                                    # (sender, hop index) -> the packet as sent

    def hop(self, t, reports=None, nacks=None):
        arrived = []
        for s in range(self.senders):
            p = wire.pack_transport(t & 0xFFFF, self.rng.integers(0, 256, wire.packet_bytes(N, T), dtype=np.uint8).tobytes(), N)
            self.originals[s, t & 0xFFFF] = p
            if self.rng.random() >= self.uplink_loss.get(s, 0.0):
                arrived.append((s, p))
        action = np.full(self.B, int(t == 0), dtype=np.int32)
        kw = {} if self.dcfg is None else dict(reports=reports, nacks=nacks)
        res = self.model.step(*arrival_arrays(arrived, self.tb), self.room, self.layers, action, **kw)
        b = self.listener
        rows = [(j, res["out"][b, j, k, :res["out_nbytes"][b, j, k]].tobytes()) for j in range(FANOUT)
                for k in range(LOOP_FORWARD.burst) if res["out_nbytes"][b, j, k] > 0]
        return rows, res


def run_rate_loop(cap, control=True, hops=3000, tail=2000, uplink_loss=None, seed=3, senders=SENDERS):
    """the closed loop of rate control: the listener's rows of a hop are offered to one SharedLink(cap), starting at route t mod fanout
    (in a fixed order drop-tail puts all loss on the last route, and the minimum over the routes then never sees it); the client is a
    3-slot JitterModel with a ReportModel, its reports come back through a ReportLine.  Returns dict(loss: the link's drops over the
    last `tail` hops as a fraction of the packets offered, kbps and layers: the listener's rate and DL_LAYERS per hop (control only),
    model)"""
    conf = Conference(DownlinkConfig(rate=LOOP_RATE) if control else None, seed, uplink_loss, senders)
    LISTENER = conf.listener
    link, line = SharedLink(cap), ReportLine()
    jm, pm = JitterModel(FANOUT, LOOP_JITTER, N, 0, T, None, conceal=True), ReportModel(FANOUT, LOOP_REPORT)
    zeros = np.zeros(FANOUT, dtype=np.int32)
    offered = dropped = 0
    rates, eff = np.zeros(hops), np.zeros(hops, dtype=np.int64)
    for t in range(hops):
        routes, blobs = line.reports_for(t)
        rows, res = conf.hop(t, reports=([LISTENER] * len(routes), routes, blobs) if control else None)
        first = next((i for i, (j, _) in enumerate(rows) if j >= t % FANOUT), 0)
        rows = rows[first:] + rows[:first]
        drops, out = link.hop_many(rows)
        if t >= hops - tail:
            offered, dropped = offered + len(rows), dropped + sum(drops)
        started = res["new_routes"][LISTENER].astype(np.int32)            # the client restarts that route's decoder slot
        jm.step(started, zeros, *arrival_arrays(out, conf.tb))
        o = pm.step(jm.state, started)
        line.push(t, [(j, o["reports"][j].tobytes()) for j in range(FANOUT) if o["due"][j]])
        if control:
            rates[t] = downlink.kbps(conf.model.downlink.state[LISTENER], T)
            eff[t] = res["eff_layers"][LISTENER]
    return dict(loss=dropped / max(offered, 1), kbps=rates, layers=eff, model=conf.model)


def run_nack_loop(answers, p_drop=0.05, hops=3000, seed=5):
    """the closed loop of NACK answers: every row for the listener, a retransmission included, is lost with probability p_drop; the
    client is a 3-slot JitterModel with a NackModel whose NACKs reach the forwarder rtt_hops later (answers=False: they are not sent);
    the retransmissions of a hop arrive behind its rows.  Returns dict(lost: STAT_LOST over the client's slots, recovered:
    NK_RECOVERED over them, sent: DL_RTX_SENT of the listener, bad: the retransmitted rows that are not the sender's original packet,
    malformed: STAT_MALFORMED over the slots)"""
    conf = Conference(DownlinkConfig(history=16, per_hop=2), seed)
    LISTENER = conf.listener
    drop = np.random.default_rng([seed, 1])
    jm, nm = JitterModel(FANOUT, LOOP_JITTER, N, 0, T, None, conceal=True), NackModel(FANOUT, LOOP_NACK, LOOP_JITTER.capacity, 0)
    zeros = np.zeros(FANOUT, dtype=np.int32)
    line, bad = {}, 0
    for t in range(hops):
        due = line.pop(t, [])
        rows, res = conf.hop(t, nacks=([LISTENER] * len(due), [j for j, _ in due], [blob for _, blob in due]))
        for q in range(conf.dcfg.per_hop):
            nb, j = int(res["rtx_nbytes"][LISTENER, q]), int(res["rtx_routes"][LISTENER, q])
            if nb > 0:
                p = res["rtx_packets"][LISTENER, q, :nb].tobytes()
                bad += p != conf.originals[int(res["routes"][LISTENER, j]), (p[0] << 8) | p[1]]
                rows.append((j, p))
        arrived = [row for row in rows if drop.random() >= p_drop]
        started = res["new_routes"][LISTENER].astype(np.int32)
        jm.step(started, zeros, *arrival_arrays(arrived, conf.tb))
        o = nm.step(jm.state, jm.meta, started)
        if answers:
            line[t + LOOP_NACK.rtt_hops] = [(j, o["nacks"][j].tobytes()) for j in range(FANOUT) if o["due"][j]]
    return dict(lost=int(jm.state[:, jitter.STAT_LOST].sum()), recovered=int(nm.state[:, rtx.NK_RECOVERED].sum()),
                sent=int(conf.model.downlink.state[LISTENER, downlink.DL_RTX_SENT]), bad=int(bad),
                malformed=int(jm.state[:, jitter.STAT_MALFORMED].sum()))
