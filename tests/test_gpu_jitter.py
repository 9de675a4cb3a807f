"""GPU: transport header and jitter buffer of the graphed sender / receiver (GraphedEncodeHop(header=True),
GraphedDecodeHop(jitter=JitterConfig(...)).play()).  The two kernels against wire.pack_transport and jitter.JitterModel, the jitter
receiver against a receiver without it driven by step(packets, n, hold, lost, fec, sid, silent) from the model's decisions, and the
headed sender through a simulated network into play() — every comparison bit for bit (torch.equal / np.array_equal)."""
import numpy as np
import pytest
import torch

from hilcodec_amd import dtx, jitter, synth, wire
from hilcodec_amd.jitter import JitterConfig, JitterModel
from tests.hops import arrival_records

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
HOP = 320


@pytest.fixture(scope="module")
def speech():
    return synth.streaming_model()


class Network:
    """seeded traffic of B senders (hop counters from `h0`): each hop every slot sends a codes packet, a SID (DTX) or nothing;
    packets are lost, delayed up to `delay` hops (reordered), duplicated or corrupted; `hold` / `start` rates give the host holds and
    the restarts (sender and receiver together) of each hop"""

    def __init__(self, B, n, m, K, T, seed, loss=0.05, delay=3, dup=0.01, bad=0.0, early=0.0, hold=0.0, start=0.0, sid=0.0, h0=None):
        self.B, self.n, self.m, self.K, self.T = B, n, m, K, T
        self.rng = np.random.default_rng(seed)
        self.tbytes = wire.transport_bytes(n, m, T)
        self.h = (self.rng.integers(0, 65536, B) if h0 is None else np.full(B, h0)).astype(np.int64)
        self.dtx = np.zeros(B, dtype=bool)
        self.rates = dict(loss=loss, delay=delay, dup=dup, bad=bad, early=early, hold=hold, start=start, sid=sid)
        self.flight = []                                     # (due hop, slot, packet bytes)
        self.k = 0

    def _packet(self, b):
        r, h = self.rng, int(self.h[b])
        if self.K is not None and (self.dtx[b] or r.random() < self.rates["sid"]):
            self.dtx[b] = r.random() < 0.8
            if r.random() < 0.4 or not self.dtx[b]:
                body = r.integers(0, 256, dtx.sid_bytes(self.K)).astype(np.uint8).tobytes()
                return wire.pack_transport(h, body, 0, sid=True) if self.dtx[b] else None
            return None                                      # silent: nothing sent
        nb = int(r.integers(max(self.m, 1), self.n + 1))
        fec = self.m >= 1 and r.random() < 0.7
        codes = torch.from_numpy(r.integers(0, 1024, (nb + (self.m if fec else 0), self.T)))
        return wire.pack_transport(h, wire.pack_stream_packet(codes), nb, fec=fec)

    def hop(self):
        """-> (slots, packets uint8 [A, tbytes], nbytes, action [B], hold [B]) of this hop"""
        r, B, k = self.rng, self.B, self.k
        action = (r.random(B) < self.rates["start"]).astype(np.int32)
        hold = (r.random(B) < self.rates["hold"]).astype(np.int32)
        for b in np.nonzero(action)[0]:
            self.h[b] = 0
            self.dtx[b] = False
        for b in range(B):
            if hold[b]:
                continue
            p = self._packet(b)
            self.h[b] = (self.h[b] + 1) & 0xFFFF
            if p is None or r.random() < self.rates["loss"]:
                continue
            for _ in range(2 if r.random() < self.rates["dup"] else 1):
                due = k + int(r.integers(0, self.rates["delay"] + 1))
                if r.random() < self.rates["early"]:
                    due = k
                    p = wire.pack_transport((self.h[b] + 20) & 0xFFFF, p[3:], p[2] & 0x1F, sid=bool(p[2] & 0x80),
                                            fec=bool(p[2] & 0x40))
                q = bytearray(p)
                nb = len(q)
                if r.random() < self.rates["bad"]:
                    how = int(r.integers(0, 3))
                    if how == 0:
                        q[2] |= 0x20
                    elif how == 1:
                        nb -= 1
                    else:
                        nb = 2
                self.flight.append((due, b, bytes(q), nb))
        now = [f for f in self.flight if f[0] <= k]
        self.flight = [f for f in self.flight if f[0] > k]
        perm = r.permutation(len(now))
        now = [now[i] for i in perm]
        pk = np.zeros((len(now), self.tbytes), dtype=np.uint8)
        for a, f in enumerate(now):
            pk[a, :len(f[2])] = np.frombuffer(f[2], dtype=np.uint8)
        self.k += 1
        return [f[1] for f in now], pk, [f[3] for f in now], action, hold


# ---------------------------------------------------------------- the kernels against wire.py / jitter.py
@pytest.mark.parametrize("T,m,dtx_on", [(1, 0, False), (1, 2, True), (2, 2, False), (3, 0, True)])
def test_packet_header_kernel(T, m, dtx_on):
    from hilcodec_amd import ops
    B, n = 96, 8
    rng = np.random.default_rng(10 * T + m)
    stride = wire.packet_bytes(n + m, T)
    for trial in range(3):
        n_b = rng.integers(max(m, 1), n + 1, B)
        kind = rng.integers(0, 4, B) if dtx_on else np.ones(B, dtype=np.int64)
        hold = (kind == dtx.HELD).astype(np.int32) if dtx_on else (rng.random(B) < 0.1).astype(np.int32)
        action = (rng.random(B) < 0.15).astype(np.int32)
        ctr = rng.integers(0, 65536, B).astype(np.int32)
        ctr[:4] = [65535, 0, 65534, 1]
        packets = np.zeros((B, stride), dtype=np.uint8)
        nbytes = np.zeros(B, dtype=np.int32)
        fec = m >= 1
        for b in range(B):
            if hold[b] or kind[b] == dtx.SILENT:
                continue
            if kind[b] == dtx.SID:
                L = dtx.sid_bytes(8)
            else:
                L = wire.fec_packet_bytes(n_b[b], m, T) if fec and rng.random() < 0.6 else wire.packet_bytes(n_b[b], T)
            packets[b, :L] = rng.integers(0, 256, L)
            nbytes[b] = L
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).to(DEV)
        c_in, c_out = t(ctr), torch.full((B,), -7, dtype=torch.int32, device=DEV)
        out, cnt = ops.packet_header(torch.from_numpy(packets).to(DEV), t(nbytes), c_in, c_out, n, m, T, n_clip=t(n_b),
                                     kind=t(kind) if dtx_on else None, action=t(action), hold=t(hold))
        want = np.zeros((B, wire.transport_bytes(n, m, T)), dtype=np.uint8)
        want_cnt = np.zeros(B, dtype=np.int32)
        want_ctr = np.zeros(B, dtype=np.int32)
        for b in range(B):
            c = 0 if action[b] else int(ctr[b])
            want_ctr[b] = c if hold[b] else (c + 1) & 0xFFFF
            if hold[b] or nbytes[b] == 0:
                continue
            if kind[b] == dtx.SID:
                pkt = wire.pack_transport(c, packets[b, :nbytes[b]].tobytes(), 0, sid=True)
            else:
                present = m >= 1 and wire.fec_present(int(nbytes[b]), int(n_b[b]), m, T)
                pkt = wire.pack_transport(c, packets[b, :nbytes[b]].tobytes(), int(n_b[b]), fec=present)
            want[b, :len(pkt)] = np.frombuffer(pkt, dtype=np.uint8)
            want_cnt[b] = len(pkt)
        assert np.array_equal(out.cpu().numpy(), want)
        assert np.array_equal(cnt.cpu().numpy(), want_cnt)
        assert np.array_equal(c_out.cpu().numpy(), want_ctr)


JITTER_CASES = [
    # (B, hops, n, m, K, T, conceal, D, C)
    (64, 200, 8, 2, 8, 1, True, 2, 8),
    (64, 200, 6, 0, None, 2, False, 1, 4),
    (64, 200, 8, 3, 4, 1, False, 0, 2),
    (64, 200, 8, 2, 8, 3, True, 14, 16),
    (1024, 30, 8, 2, 8, 1, True, 3, 32),
]


@pytest.mark.parametrize("case", JITTER_CASES)
def test_jitter_step_kernel(case):
    from hilcodec_amd import ops
    B, hops, n, m, K, T, conceal, D, C = case
    cfg = JitterConfig(depth=D, capacity=C)
    model = JitterModel(B, cfg, n, m, T, K, conceal)
    net = Network(B, n, m, K, T, seed=B + hops + C, loss=0.05, delay=C, dup=0.02, bad=0.02, early=0.01, hold=0.03, start=0.01,
                  sid=0.05 if K is not None else 0.0)
    net.h[:8] = 65530                                        # these cross the 16-bit wrap early
    stride = wire.packet_bytes(n + m, T)
    rw = (stride + 3) // 4
    state = torch.zeros(B, jitter.ST_WORDS, dtype=torch.int32, device=DEV)
    meta = torch.zeros(B, C, dtype=torch.int32, device=DEV)
    ring = torch.zeros(B, C, rw, dtype=torch.int32, device=DEV)
    rows = torch.zeros(3, B, dtype=torch.int32, device=DEV)
    pk = torch.zeros(B, stride, dtype=torch.uint8, device=DEV)
    for k in range(hops):
        slots, packets, nbytes, action, hold = net.hop()
        assert len(slots) <= 2 * B
        arr, offs = arrival_records(slots, packets, nbytes, net.tbytes, B, 2 * B)
        hold_d = torch.from_numpy(hold).to(DEV)
        rows.fill_(-9)
        pk.fill_(0xEE)
        ops.jitter_step(arr, offs, hold_d, rows[0], pk, state, meta, ring, n, m, T, K, D, action=torch.from_numpy(action).to(DEV),
                        lost=rows[1] if conceal else None, fec=rows[2] if m else None)
        want = model.step(action, hold, slots, packets, nbytes)
        assert np.array_equal(hold_d.cpu().numpy(), want["hold"]), k
        assert np.array_equal(rows[0].cpu().numpy(), want["n"]), k
        if conceal:
            assert np.array_equal(rows[1].cpu().numpy(), want["lost"]), k
        if m:
            assert np.array_equal(rows[2].cpu().numpy(), want["fec"]), k
        assert np.array_equal(pk.cpu().numpy(), want["packets"]), k
        assert np.array_equal(state.cpu().numpy(), model.state), k
        assert np.array_equal(meta.cpu().numpy(), model.meta), k
    st = model.state
    for name in ("accepted", "decoded", "lost", "late", "malformed", "duplicate"):
        assert st[:, jitter.STAT_ACCEPTED + jitter.STAT_NAMES.index(name)].sum() > 0, name
    if m:
        assert st[:, jitter.STAT_FEC].sum() > 0
    if K is not None:
        assert st[:, jitter.STAT_NOISE].sum() > 0


# ---------------------------------------------------------------- play() against the explicit step()
def explicit_step(rx, rows, hold_host):
    """drive a receiver without jitter with the model's decisions"""
    hv = rows["hold"]
    kw = dict(hold=np.nonzero(hv == 1)[0].tolist())
    if rx.conceal:
        kw["lost"] = np.nonzero(rows["lost"])[0].tolist()
    if rx.fec_stages:
        kw["fec"] = np.nonzero(rows["fec"])[0].tolist()
    if rx.cng_order is not None:
        kw["sid"] = np.nonzero(hv == 2)[0].tolist()
        kw["silent"] = np.nonzero(hv == 3)[0].tolist()
    return rx.step(torch.from_numpy(rows["packets"]), rows["n"].tolist(), **kw)


def compare(a, b, k):
    for x, y in zip(a.cache_dec, b.cache_dec):
        assert torch.equal(x, y), k
    if a.conceal:
        assert torch.equal(a.concealed, b.concealed), k
    if a.cng_order is not None:
        assert torch.equal(a.cng_state, b.cng_state), k


PLAY_CASES = [
    dict(),
    dict(conceal=True),
    dict(conceal=True, fec_stages=2),
    dict(conceal=True, fec_stages=2, cng_order=8),
    dict(conceal=True, fec_stages=2, cng_order=8, output_rate=48000),
    dict(conceal=True, fec_stages=2, cng_order=8, frames=2),
    dict(frames=2),
]


@pytest.mark.parametrize("kw", PLAY_CASES, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()) or "sessions")
def test_play_matches_explicit_step(speech, kw):
    from hilcodec_amd.graph_step import GraphedDecodeHop
    kw = dict(kw)
    B, n, hops = 12, 8, 40
    T = kw.pop("frames", 1)
    cfg = JitterConfig(depth=2, capacity=8)
    jx = GraphedDecodeHop(speech, B, T, n, DEV, sessions=True, jitter=cfg, **kw)
    ex = GraphedDecodeHop(speech, B, T, n, DEV, sessions=True, **kw)
    m, K = kw.get("fec_stages", 0), kw.get("cng_order")
    model = JitterModel(B, cfg, n, m, T, K, kw.get("conceal", False))
    net = Network(B, n, m, K, T, seed=3, loss=0.08, delay=3, dup=0.02, bad=0.02, hold=0.04, start=0.02, sid=0.08 if K else 0.0)
    on_device = False
    for k in range(hops):
        slots, packets, nbytes, action, hold = net.hop()
        for b in np.nonzero(action)[0]:
            jx.start(int(b))
            ex.start(int(b))
        rows = model.step(action, hold, slots, packets, nbytes)
        host_hold = np.nonzero(hold)[0].tolist()
        pk = torch.from_numpy(packets)
        on_device = not on_device
        a = jx.play(slots, pk.to(DEV) if on_device else pk, nbytes, hold=host_hold).clone()
        b = explicit_step(ex, rows, host_hold).clone()
        assert torch.equal(a, b), k
        compare(jx, ex, k)
        assert np.array_equal(jx.jitter_state.cpu().numpy(), model.state), k
    torch.cuda.synchronize()
    st = model.state
    assert st[:, jitter.STAT_DECODED].sum() > 0 and st[:, jitter.STAT_LOST].sum() > 0
    # export carries no jitter state: the same caches as the explicit receiver's
    for x, y in zip(jx.export(3), ex.export(3)):
        assert torch.equal(x, y)
    # start clears a slot's jitter state (no arrival for it on that hop)
    jx.start(3)
    jx.play([], torch.zeros(0, jx.tstride, dtype=torch.uint8), [])
    assert not jx.jitter_state[3].any() and jx.jitter_state.any()
    with pytest.raises(RuntimeError):
        jx.step(torch.zeros(B, jx.stride, dtype=torch.uint8), [n] * B)
    with pytest.raises(RuntimeError):
        ex.play([], torch.zeros(0, jx.tstride, dtype=torch.uint8), [])
    with pytest.raises(IndexError):
        jx.play([B], torch.zeros(1, jx.tstride, dtype=torch.uint8), [3])
    with pytest.raises(ValueError):
        jx.play([0] * (2 * B + 1), torch.zeros(2 * B + 1, jx.tstride, dtype=torch.uint8), [3] * (2 * B + 1))


def test_jitter_receiver_arguments(speech):
    from hilcodec_amd.graph_step import GraphedDecodeHop
    with pytest.raises(ValueError):
        GraphedDecodeHop(speech, 4, 1, 8, DEV, jitter=JitterConfig())                     # needs sessions
    with pytest.raises(ValueError):
        GraphedDecodeHop(speech, 4, 1, 8, DEV, sessions=True, jitter=(2, 8))
    with pytest.raises(ValueError):
        GraphedDecodeHop(speech, 4, 1, 8, DEV, sessions=True, max_arrivals=8)            # max_arrivals without jitter


# ---------------------------------------------------------------- end to end: the headed sender through a network into play()
def audio(B, hops, seed):
    """noise bursts with silent stretches (digital zero) of a few to many hops"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, hops * HOP, generator=g) * 0.1
    on = torch.ones(B, hops)
    for b in range(B):
        k = int(b % 5)
        while k < hops:
            L = 3 + (b * 7 + k) % 23
            on[b, k:k + L] = 0
            k += L + 4 + (b + k) % 9
    return (x.view(B, hops, HOP) * on[:, :, None]).view(B, hops * HOP)


def test_end_to_end_headed_sender_into_play(speech):
    from hilcodec_amd.graph_step import GraphedDecodeHop, GraphedEncodeHop
    B, n, m, hops, D = 8, 8, 2, 60, 2
    cfg_dtx = dtx.DtxConfig(hangover=2, sid_interval=4)
    tx = GraphedEncodeHop(speech, B, HOP, n, DEV, sessions=True, fec_stages=m, dtx=cfg_dtx, header=True)
    tp = GraphedEncodeHop(speech, B, HOP, n, DEV, sessions=True, fec_stages=m, dtx=cfg_dtx)
    rkw = dict(sessions=True, conceal=True, fec_stages=m, cng_order=cfg_dtx.order)
    cfg = JitterConfig(depth=D, capacity=8)
    jx = GraphedDecodeHop(speech, B, 1, n, DEV, jitter=cfg, **rkw)
    ex = GraphedDecodeHop(speech, B, 1, n, DEV, **rkw)
    x = audio(B, hops, 5).to(DEV)
    # a perfect network: the same audio out, D hops later
    ref, got, kinds = [], [], []
    for k in range(hops):
        xk = x[:, k * HOP:(k + 1) * HOP].reshape(B, 1, HOP)
        pk, nb = tx.step(xk)
        pk, nb = pk.clone(), nb.cpu().numpy()
        pp, nbp = tp.step(xk)
        kind = tp.kind.cpu().numpy()
        kinds.append(kind)
        assert np.array_equal(nb, np.where(nbp.cpu().numpy() > 0, nbp.cpu().numpy() + 3, 0)), k
        assert torch.equal(pk[:, 3:], torch.where(torch.from_numpy(nb > 0).to(DEV)[:, None], pp, torch.zeros_like(pp))), k
        assert np.array_equal(tx.hop_index.cpu().numpy(), np.full(B, k + 1)), k
        sent = np.nonzero(nb > 0)[0]
        got.append(jx.play(sent.tolist(), pk[torch.from_numpy(sent).to(DEV)], nb[sent].tolist()).clone())
        sid = np.nonzero(kind == dtx.SID)[0].tolist()
        silent = np.nonzero(kind == dtx.SILENT)[0].tolist()
        ref.append(ex.step(pp, [n] * B, sid=sid, silent=silent).clone())
    assert sum(int((kd == dtx.SILENT).sum()) for kd in kinds) > 0 and sum(int((kd == dtx.SID).sum()) for kd in kinds) > 0
    for k in range(D):
        assert not got[k].any(), k
    for k in range(hops - D):
        assert torch.equal(got[k + D], ref[k]), k
    # a lossy network (5 % loss, reordering, duplicates): the explicit receiver driven by the model's decisions
    for b in range(B):
        tx.start(b)
        jx.start(b)
        ex.start(b)
    model = JitterModel(B, cfg, n, m, 1, cfg_dtx.order, True)
    rng = np.random.default_rng(11)
    flight = []
    action = np.ones(B, dtype=np.int32)
    for k in range(hops):
        xk = x[:, k * HOP:(k + 1) * HOP].reshape(B, 1, HOP)
        pk, nb = tx.step(xk)
        pk, nb = pk.cpu().numpy(), nb.cpu().numpy()
        for b in np.nonzero(nb > 0)[0]:
            if rng.random() < 0.05:
                continue
            for _ in range(2 if rng.random() < 0.02 else 1):
                flight.append((k + int(rng.integers(0, D + 1)), int(b), pk[b].copy(), int(nb[b])))
        now = [f for f in flight if f[0] <= k]
        flight = [f for f in flight if f[0] > k]
        now = [now[i] for i in rng.permutation(len(now))]
        slots = [f[1] for f in now]
        packets = np.stack([f[2] for f in now]) if now else np.zeros((0, jx.tstride), dtype=np.uint8)
        nbytes = [f[3] for f in now]
        rows = model.step(action, np.zeros(B, dtype=np.int32), slots, packets, nbytes)
        a = jx.play(slots, torch.from_numpy(packets), nbytes).clone()
        b = explicit_step(ex, rows, []).clone()
        assert torch.equal(a, b), k
        compare(jx, ex, k)
        action[:] = 0
    st = model.state
    assert st[:, jitter.STAT_LOST].sum() + st[:, jitter.STAT_FEC].sum() > 0 and st[:, jitter.STAT_NOISE].sum() > 0
