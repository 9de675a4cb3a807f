"""GPU: in-band forward error correction of the graphed sender / receiver (GraphedEncodeHop(fec_stages=m),
GraphedDecodeHop(fec_stages=m), `step(..., fec=slots)`).  The two kernels against host models, the sender against a sender
without FEC and the wire definition of its packets, the receiver against a receiver without FEC fed `wire.fec_primary` /
`wire.fec_redundant` rows — every comparison bit for bit (torch.equal), except the oracle leg (the project's waveform bar, 1e-4)."""
import numpy as np
import pytest
import torch

from hilcodec_amd import synth, wire
from hilcodec_amd.resample import hop_samples
from tests.hops import build_streaming, caches_equal, pack_model, put_row, row_bytes, select_model

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
HOP = 320
M = 2


@pytest.fixture(scope="module")
def built():
    return build_streaming()


@pytest.fixture(scope="module")
def speech(built):
    return built[0]


# ---------------------------------------------------------------- the kernels against host models


@pytest.mark.parametrize("B", [37, 1024])
@pytest.mark.parametrize("T", [1, 2, 3])
@pytest.mark.parametrize("n_max,m", [(8, 2), (12, 4), (3, 3)])
def test_pack_fec_kernel(B, T, n_max, m):
    from hilcodec_amd import ops
    gen = torch.Generator().manual_seed(B + 10 * T + 100 * n_max + m)
    W = 1 + m * T
    for trial in range(3):
        idx = torch.randint(-2, 1100, (n_max, B, T), generator=gen)              # outside [0, 1024): clamped
        n_slot = torch.randint(0, n_max + 2, (B,), generator=gen, dtype=torch.int32)   # clamped to [m, n_max]
        prev_in = torch.randint(0, 2048, (B, W), generator=gen, dtype=torch.int32)    # codes past 10 bits: masked
        prev_in[:, 0] = torch.randint(0, 3, (B,), generator=gen)                      # any non-zero is valid
        action = torch.randint(-1, 3, (B,), generator=gen, dtype=torch.int32) * (torch.randint(0, 4, (B,), generator=gen) == 0)
        hold = (torch.randint(0, 5, (B,), generator=gen) == 0).to(torch.int32)
        exp = pack_model(idx, n_slot, prev_in, action, hold, m)
        d = [t.to(DEV) for t in (idx, n_slot, prev_in, action, hold)]
        prev_out = torch.full((B, W), 77, dtype=torch.int32, device=DEV)
        pk, nb = ops.pack_codes_10bit_fec(d[0], d[2], prev_out, m, d[1], d[3], d[4])
        torch.cuda.synchronize()
        for name, g, e in zip(("packets", "nbytes", "prev_out"), (pk.cpu(), nb.cpu(), prev_out.cpu()), exp):
            assert torch.equal(g, e), f"trial {trial}: {name}"
        assert torch.equal(d[2].cpu(), prev_in)                                       # read-only
    # no action / hold rows, every n = n_max (the sessions=False sender)
    prev_in = torch.zeros(B, W, dtype=torch.int32)
    prev_in[::2, 0] = 1
    prev_in[:, 1:] = torch.randint(0, 1024, (B, W - 1), generator=gen, dtype=torch.int32)
    idx = torch.randint(0, 1024, (n_max, B, T), generator=gen)
    z = torch.zeros(B, dtype=torch.int32)
    exp = pack_model(idx, torch.full((B,), n_max, dtype=torch.int32), prev_in, z, z, m)
    prev_out = torch.zeros(B, W, dtype=torch.int32, device=DEV)
    pk, nb = ops.pack_codes_10bit_fec(idx.to(DEV), prev_in.to(DEV), prev_out, m)
    assert torch.equal(pk.cpu(), exp[0]) and torch.equal(nb.cpu(), exp[1]) and torch.equal(prev_out.cpu(), exp[2])


@pytest.mark.parametrize("B", [37, 1024])
@pytest.mark.parametrize("T", [1, 2, 3])
@pytest.mark.parametrize("n_max,m", [(8, 2), (12, 4), (3, 3), (8, 1)])
def test_select_kernel(B, T, n_max, m):
    from hilcodec_amd import ops
    gen = torch.Generator().manual_seed(B + 10 * T + 100 * n_max + m)
    for trial in range(3):
        wide = torch.randint(0, 256, (B, wire.fec_packet_bytes(n_max, m, T)), generator=gen, dtype=torch.uint8)  # every bit set at random
        fec = (torch.randint(0, 3, (B,), generator=gen) == 0).to(torch.int32) * torch.randint(1, 3, (B,), generator=gen, dtype=torch.int32)
        n_slot = torch.randint(-1, n_max + 3, (B,), generator=gen, dtype=torch.int32)          # garbage: clamped
        exp, n_exp = select_model(wide, fec, n_slot, n_max, m, T)
        d_wide, d_fec, d_n = wide.to(DEV), fec.to(DEV), n_slot.to(DEV)
        out = ops.fec_select(d_wide, d_fec, d_n, n_max, m, T)
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), exp), f"trial {trial}: rows"
        assert torch.equal(d_n.cpu(), n_exp), f"trial {trial}: n"
        assert torch.equal(d_wide.cpu(), wide) and torch.equal(d_fec.cpu(), fec)


# ---------------------------------------------------------------- the sender
def run_sender_plan(model, B, frames, hops, seed, n=8, input_rate=24000):
    """FEC sender (m = M) against a sender without FEC: starts, a resume, holds, a started-and-held slot, a stop and restart,
    set_bitrate (to m and above); both sessions=True"""
    from hilcodec_amd.graph_step import GraphedEncodeHop
    T = frames
    n_in = hop_samples(frames, input_rate)
    x = synth.synth_clips(B, n_in * hops, seed=seed).to(DEV)
    kw = dict(sessions=True, input_rate=input_rate)
    f = GraphedEncodeHop(model, B, HOP * frames, n, DEV, fec_stages=M, **kw)
    p = GraphedEncodeHop(model, B, HOP * frames, n, DEV, **kw)
    rng = np.random.default_rng(seed)
    nb = [n] * B
    prev = [None] * B                                    # each slot's last encoded hop's first M stages
    for h in range(hops):
        fresh, hold = set(), set()
        if h == 2:
            for s in (f, p):
                s.start(3)
                s.start(4, n=4)
            fresh |= {3, 4}
            nb[3], nb[4] = n, 4
        if h == 3:
            hold |= {5, 6, 7}
            for s in (f, p):
                s.start(7)                               # started and held on the same hop: the fresh state, no previous hop
            fresh.add(7)
            nb[7] = n
        if h == 4:
            for s in (f, p):
                s.stop(8)
        if h == 5:
            for s in (f, p):
                s.start(9, s.export(10), n=3)            # a resume carries no FEC state
            fresh.add(9)
            nb[9] = 3
        if h == 6:
            for s in (f, p):
                s.set_bitrate(11, M)
                s.set_bitrate(12, 5)
            nb[11], nb[12] = M, 5
        if h == 8:
            for s in (f, p):
                s.start(8, n=6)                          # restart after the stop
            fresh.add(8)
            nb[8] = 6
        if h >= 1:
            hold |= set(rng.choice(np.arange(20, B), size=2, replace=False).tolist())
        chunk = x[:, :, n_in * h:n_in * (h + 1)].contiguous()
        pk, nbytes = f.step(chunk, hold=sorted(hold))
        pk0, nbytes0 = p.step(chunk, hold=sorted(hold))
        assert torch.equal(f.indices, p.indices), f"hop {h}: indices"
        assert pk.shape == (B, wire.fec_packet_bytes(n, M, T)) and pk0.shape == (B, wire.packet_bytes(n, T))
        idx = f.indices.cpu()
        pk, nbytes, pk0, nbytes0 = pk.cpu(), nbytes.cpu(), pk0.cpu(), nbytes0.cpu()
        held = hold | set(f.stopped)
        for b in range(B):
            if b in fresh:
                prev[b] = None
            if b in held:
                assert int(nbytes[b]) == 0 and not bool(pk[b].any()), f"hop {h} slot {b}: held"
                continue
            exp = wire.pack_fec_packet(idx[:nb[b], b], prev[b])
            got = row_bytes(pk, b, int(nbytes[b]))
            assert got == exp, f"hop {h} slot {b}"
            assert not bool(pk[b, len(exp):].any()), f"hop {h} slot {b}: past the packet"
            assert wire.fec_present(len(got), nb[b], M, T) == (prev[b] is not None)
            assert wire.fec_primary(got, nb[b], T) == row_bytes(pk0, b, int(nbytes0[b])), f"hop {h} slot {b}: primary"
            prev[b] = idx[:M, b].clone()
    assert sum(p is not None for p in prev) > B // 2
    return f


@pytest.mark.parametrize("B,frames", [(37, 2), (1024, 1)])
def test_sender_fec(speech, B, frames):
    run_sender_plan(speech, B, frames, hops=12, seed=B + frames)


def test_sender_fec_input_rate(speech):
    run_sender_plan(speech, 37, 1, hops=6, seed=81, input_rate=48000)


def test_sender_fec_no_sessions_and_reset(speech):
    """sessions=False: the first hop has no redundant section, every later one has; reset() forgets the previous hop"""
    from hilcodec_amd.graph_step import GraphedEncodeHop
    B, hops = 5, 4
    x = synth.synth_clips(B, HOP * hops, seed=82).to(DEV)
    f = GraphedEncodeHop(speech, B, HOP, 8, DEV, fec_stages=3)
    p = GraphedEncodeHop(speech, B, HOP, 8, DEV)
    for rnd in range(2):
        prev = None
        for h in range(hops):
            chunk = x[:, :, HOP * h:HOP * (h + 1)].contiguous()
            pk, nb = f.step(chunk)
            p.step(chunk)
            assert torch.equal(f.indices, p.indices)
            idx = f.indices.cpu()
            for b in range(B):
                exp = wire.pack_fec_packet(idx[:, b], None if prev is None else prev[:, b])
                assert row_bytes(pk.cpu(), b, int(nb[b])) == exp, (rnd, h, b)
            prev = idx[:3].clone()
        f.reset()
        p.reset()


# ---------------------------------------------------------------- the receiver
class Reference:
    """a receiver without FEC fed what FEC amounts to: `wire.fec_primary` rows for received slots, `wire.fec_redundant` rows with
    n = m for FEC slots; lost slots are concealed (conceal=True) or held (conceal=False)"""

    def __init__(self, model, B, frames, n, m, conceal, sessions=True, output_rate=24000):
        from hilcodec_amd.graph_step import GraphedDecodeHop
        self.r = GraphedDecodeHop(model, B, frames, n, DEV, sessions=sessions, conceal=conceal, output_rate=output_rate)
        self.B, self.T, self.n, self.m, self.conceal = B, frames, n, m, conceal

    def step(self, rows, n_in, hold=(), lost=(), fec=()):
        pk = torch.zeros(self.B, wire.packet_bytes(self.n, self.T), dtype=torch.uint8)
        n_list = list(n_in)
        for b in range(self.B):
            if b in hold or b in lost or b in self.r.stopped:
                continue
            if b in fec:
                put_row(pk, b, wire.fec_redundant(rows[b], n_in[b], self.m, self.T))
                n_list[b] = self.m
            else:
                put_row(pk, b, wire.fec_primary(rows[b], n_in[b], self.T))
        if self.conceal:
            return self.r.step(pk, n_list, hold=sorted(hold), lost=sorted(lost))
        return self.r.step(pk, n_list, hold=sorted(set(hold) | set(lost))) if self.r.sessions else self.r.step(pk, n_list)


class Stream:
    """per slot, a random code sequence (n_b >= m per hop) and its FEC packets: packet h carries hop h - 1's first m stages
    (packet 0 none)"""

    def __init__(self, B, T, n, m, hops, gen):
        self.T, self.m = T, m
        self.nb = torch.randint(m, n + 1, (hops + 1, B), generator=gen).tolist()
        self.codes = [[torch.randint(0, 1024, (self.nb[h][b], T), generator=gen) for b in range(B)] for h in range(hops + 1)]

    def packet(self, h, b):
        prev = None if h == 0 else self.codes[h - 1][b][:self.m]
        return wire.pack_fec_packet(self.codes[h][b], prev)


def upload(B, n, m, T, rows, gen):
    pk = torch.randint(0, 256, (B, wire.fec_packet_bytes(n, m, T)), generator=gen, dtype=torch.uint8)   # garbage past the packet
    for b, blob in rows.items():
        pk[b, :len(blob)] = torch.frombuffer(bytearray(blob), dtype=torch.uint8)
    return pk


def _compare(c, ref, wav, ref_wav, h):
    assert torch.equal(wav.cpu(), ref_wav.cpu()), f"hop {h}: wav"
    assert caches_equal(c.cache_dec, ref.r.cache_dec), f"hop {h}: caches"
    if c.conceal:
        assert torch.equal(c.concealed.cpu(), ref.r.concealed.cpu()), f"hop {h}: concealed"


def run_receiver_plan(model, B, frames, conceal, hops, seed, n=8, output_rate=24000):
    """slot 2: an isolated loss recovered by FEC (hop 3); slot 5: lost at hops 2-3, FEC at 4 (with conceal: the fade-in from
    G[2]); slot 9: started at hop 4 and FEC there; slot 13 held at hop 5 beside slot 14 FEC; slot 20 stopped at hop 3 (started
    again at 7) beside slot 21 FEC at hops 4 and 6; from hop 1 on a random few lost and a random few FEC every hop"""
    from hilcodec_amd.graph_step import GraphedDecodeHop
    gen = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    T = frames
    st = Stream(B, T, n, M, hops, gen)
    c = GraphedDecodeHop(model, B, frames, n, DEV, sessions=True, conceal=conceal, fec_stages=M, output_rate=output_rate)
    ref = Reference(model, B, frames, n, M, conceal, output_rate=output_rate)
    special = {2, 5, 9, 13, 14, 20, 21}
    pool = [b for b in range(B) if b not in special]
    for h in range(hops):
        hold, lost, fec = set(), set(), set()
        if h >= 1:
            pick = rng.choice(pool, size=2 * max(2, B // 16), replace=False).tolist()
            lost |= set(pick[:len(pick) // 2])
            fec |= set(pick[len(pick) // 2:])
        if h == 3:
            fec.add(2)
        if h in (2, 3):
            lost.add(5)
        if h == 4:
            fec.add(5)
            for side in (c, ref.r):
                side.start(9)
            fec.add(9)
        if h == 5:
            hold.add(13)
            fec.add(14)
        if h == 3:
            for side in (c, ref.r):
                side.stop(20)
        if h == 7:
            for side in (c, ref.r):
                side.start(20)
        if h in (4, 6):
            fec.add(21)
        held = hold | set(c.stopped)
        rows = {b: st.packet(h + 1 if b in fec else h, b) for b in range(B) if b not in held | lost}
        n_in = [0] * B
        for b in rows:
            n_in[b] = st.nb[h + 1][b] if b in fec else st.nb[h][b]
        pk = upload(B, n, M, T, rows, gen)
        ref_wav = ref.step(rows, n_in, hold=hold, lost=lost, fec=fec)
        if conceal:
            wav = c.step(pk.to(DEV) if h % 2 else pk, n_in, hold=sorted(hold), lost=sorted(lost), fec=sorted(fec))
        else:
            wav = c.step(pk.to(DEV) if h % 2 else pk, n_in, hold=sorted(hold | lost), fec=sorted(fec))
        _compare(c, ref, wav, ref_wav, h)
        assert bool(torch.isfinite(wav).all())
        if conceal and h == 3:
            assert int(c.concealed[5]) == 2
        if conceal and h == 4:
            assert int(c.concealed[5]) == 0
    return c, ref


@pytest.mark.parametrize("B,frames,conceal", [(37, 1, True), (37, 1, False), (37, 2, True), (37, 2, False), (1024, 1, True),
                                              (1024, 2, False)])
def test_receiver_fec_equals_reference(speech, B, frames, conceal):
    run_receiver_plan(speech, B, frames, conceal, hops=10, seed=B + 10 * frames + conceal)


def test_receiver_fec_output_rate(speech):
    run_receiver_plan(speech, 37, 1, True, hops=6, seed=91, output_rate=48000)


def test_receiver_fec_no_sessions(speech):
    """sessions=False, conceal=False: FEC slots against a plain receiver without sessions"""
    from hilcodec_amd.graph_step import GraphedDecodeHop
    B, T, n, hops = 11, 2, 8, 5
    gen = torch.Generator().manual_seed(92)
    st = Stream(B, T, n, M, hops, gen)
    c = GraphedDecodeHop(speech, B, T, n, DEV, fec_stages=M)
    ref = Reference(speech, B, T, n, M, False, sessions=False)
    for h in range(hops):
        fec = {h % B, (3 * h + 1) % B} if h else set()
        rows = {b: st.packet(h + 1 if b in fec else h, b) for b in range(B)}
        n_in = [st.nb[h + 1][b] if b in fec else st.nb[h][b] for b in range(B)]
        ref_wav = ref.step(rows, n_in, fec=fec)
        wav = c.step(upload(B, n, M, T, rows, gen), n_in, fec=sorted(fec))
        _compare(c, ref, wav, ref_wav, h)


def test_production_shape(speech):
    """sender (m = 2) -> receiver at 1 024 streams, n = 8, conceal=True, 10 % of the packets dropped each hop: FEC wherever the
    next packet arrived (and carries a redundant section), `lost` otherwise"""
    from hilcodec_amd.graph_step import GraphedDecodeHop, GraphedEncodeHop
    B, hops, n = 1024, 8, 8
    x = synth.synth_clips(B, HOP * (hops + 1), seed=93).to(DEV)
    rng = np.random.default_rng(94)
    s = GraphedEncodeHop(speech, B, HOP, n, DEV, fec_stages=M)
    sent = []
    for h in range(hops + 1):
        pk, nb = s.step(x[:, :, HOP * h:HOP * (h + 1)].contiguous())
        sent.append((pk.cpu().clone(), nb.cpu().clone()))
    drops = [set(rng.permutation(B)[:B // 10].tolist()) for _ in range(hops + 1)]
    c = GraphedDecodeHop(speech, B, 1, n, DEV, sessions=True, conceal=True, fec_stages=M)
    ref = Reference(speech, B, 1, n, M, True)
    n_fec = 0
    for h in range(hops):
        lost, fec, rows = set(), set(), {}
        for b in range(B):
            if b not in drops[h]:
                rows[b] = row_bytes(sent[h][0], b, int(sent[h][1][b]))
            elif b not in drops[h + 1] and wire.fec_present(int(sent[h + 1][1][b]), n, M, 1):
                fec.add(b)
                rows[b] = row_bytes(sent[h + 1][0], b, int(sent[h + 1][1][b]))
            else:
                lost.add(b)
        n_in = [0 if b in lost else n for b in range(B)]
        pk = torch.zeros(B, wire.fec_packet_bytes(n, M, 1), dtype=torch.uint8)
        for b, blob in rows.items():
            put_row(pk, b, blob)
        ref_wav = ref.step(rows, n_in, lost=lost, fec=fec)
        wav = c.step(pk.to(DEV), n_in, lost=sorted(lost), fec=sorted(fec))
        _compare(c, ref, wav, ref_wav, h)
        assert bool(torch.isfinite(wav).all())
        n_fec += len(fec)
    assert n_fec > hops * B // 20


def test_oracle_leg(built):
    """3 streams on the CPU oracle: a FEC-recovered hop is stream_dequantize + stream_decoder of the m redundant codes, within 1e-4"""
    from hilcodec_amd.graph_step import GraphedDecodeHop
    from oracle import hilcodec_oracle as O
    model, mk, sd = built
    p = O.stream_prepare(sd, mk)
    B, T, n, hops = 3, 1, 8, 6
    gen = torch.Generator().manual_seed(95)
    st = Stream(B, T, n, M, hops, gen)
    fec_plan = {0: [], 1: [0], 2: [1, 2], 3: [], 4: [0, 2], 5: [1]}
    c = GraphedDecodeHop(model, B, T, n, DEV, fec_stages=M)
    oc = [O.stream_init_cache(mk, 1)[1] for _ in range(B)]
    for h in range(hops):
        fec = fec_plan[h]
        rows = {b: st.packet(h + 1 if b in fec else h, b) for b in range(B)}
        n_in = [st.nb[h + 1][b] if b in fec else st.nb[h][b] for b in range(B)]
        wav = c.step(upload(B, n, M, T, rows, gen), n_in, fec=fec).cpu()
        for b in range(B):
            if b in fec:
                codes, nb = wire.unpack_stream_packet(wire.fec_redundant(rows[b], n_in[b], M, T), M, T), M
                assert torch.equal(codes, st.codes[h][b][:M])
            else:
                codes, nb = st.codes[h][b], n_in[b]
            wo, oc[b] = O.stream_decoder(p, mk, O.stream_dequantize(p, codes.reshape(nb, 1, T).long(), nb), oc[b])
            assert (wav[b:b + 1] - wo).abs().max() < 1e-4, f"hop {h} stream {b}"


def test_fec_checks(speech):
    from hilcodec_amd.graph_step import GraphedDecodeHop, GraphedEncodeHop
    B = 3
    for bad in (-1, 9, 1.5, True):
        with pytest.raises(ValueError):
            GraphedEncodeHop(speech, B, HOP, 8, DEV, fec_stages=bad)
        with pytest.raises(ValueError):
            GraphedDecodeHop(speech, B, 1, 8, DEV, fec_stages=bad)
    s = GraphedEncodeHop(speech, B, HOP, 8, DEV, sessions=True, fec_stages=3)
    for bad in (1, 2):
        with pytest.raises(ValueError):
            s.start(0, n=bad)
        with pytest.raises(ValueError):
            s.set_bitrate(0, bad)
    s.start(0, n=3)
    s.set_bitrate(1, 3)
    pk = torch.zeros(B, wire.packet_bytes(8, 1), dtype=torch.uint8)
    plain = GraphedDecodeHop(speech, B, 1, 8, DEV, sessions=True)
    with pytest.raises(RuntimeError):
        plain.step(pk, [8] * B, fec=[1])                                           # constructed without FEC
    plain.step(pk, [8] * B, fec=[])
    wide = torch.zeros(B, wire.fec_packet_bytes(8, M, 1), dtype=torch.uint8)
    c = GraphedDecodeHop(speech, B, 1, 8, DEV, sessions=True, conceal=True, fec_stages=M)
    before = c.cache_dec[0].clone()
    with pytest.raises(ValueError):
        c.step(pk, [8] * B)                                                        # rows of the narrow width
    with pytest.raises(ValueError):
        c.step(wide, [8] * B, hold=[1], fec=[1])                                   # fec and held
    with pytest.raises(ValueError):
        c.step(wide, [8] * B, lost=[1], fec=[1])                                   # fec and lost
    with pytest.raises(IndexError):
        c.step(wide, [8] * B, fec=[3])
    with pytest.raises(ValueError):
        c.step(wide, [8] * B, fec=torch.tensor([1], device=DEV))                   # host ints only
    with pytest.raises(ValueError):
        c.step(wide, [8, M - 1, 8], fec=[1])                                       # the next packet's n must be >= m
    with pytest.raises(ValueError):
        c.step(wide, [8, 9, 8], fec=[1])
    c.stop(2)
    with pytest.raises(ValueError):
        c.step(wide, [8] * B, fec=[2])                                             # stopped
    assert c.parity == 0 and torch.equal(c.cache_dec[0], before)                   # nothing was launched
    c.step(wide, [8, M, 8], fec=[1])
    c.step(wide, [M - 1, 8, 8], lost=[0], fec=[1])                                 # a lost slot's n is not checked
