"""GPU: quality-targeted variable bitrate of the graphed sender (GraphedEncodeHop(vbr=VbrConfig(...))).  The kernel against
hilcodec_amd/vbr.py, the sender against an eager composition (the same model's streaming encoder, its quantiser, vbr.VbrModel, the
wire packers), the packets through the unchanged receiver — every comparison bit for bit (torch.equal).

Two notes on the inputs.
  * The constructed kernel family takes codebooks[s] = randn 0.9^s.  With randn 2^-s the error after s stages is about 4^-s of the
    input's energy, which is under the 20 dB bar from s = 4 on, so a slot built from d_b > 4 stages could not be expected to stop at
    d_b; with 0.9^s the last of d_b <= 12 stages still holds 2 % of the energy and n_eff = d_b is asserted for every slot.  The
    2^-s family runs as well, compared bit for bit.
  * The sender tests load per-stage codebooks randn(1024, 128) g 0.95^s into the quantiser and the dequantiser (with the synthetic
    model's plain randn codebooks a stage does not reduce the error and the rule never fires).  The encoder ends in an L2 norm with
    scale sqrt(128), so g is 0.05 times the measured norm of the latents rather than 0.05: at g = 0.05 a stage removes so little of
    a latent of norm 11.3 that every slot stops within two neighbouring stage counts.  The decay is 0.95 rather than 0.9: measured
    on this model's latents, 0.9^s leaves a three-frame hop (whose D averages over the frames) with two values of n_eff over 48
    decisions, 0.95^s with four, and a one-frame hop with seven.  rho is the reference's own median of D[:, n / 2] / D[:, 0] at
    hop 0, and every sender test asserts on the reference that n_eff takes at least 3 values among the slots that are neither
    held nor under a lower ceiling."""
import pytest
import torch

from hilcodec_amd import dtx, synth, vbr, wire
from hilcodec_amd.jitter import JitterConfig
from hilcodec_amd.resample import design, hop_samples, reference
from hilcodec_amd.vbr import VbrConfig, VbrModel
from tests.hops import target_from_reference, vbr_speech_model

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
HOP = 320
C, K = 128, 1024


# ---------------------------------------------------------------- the kernel against vbr.py
def run_kernel(cfg, z, idx, cb, n_b, action, hold, credit, T, fec=0):
    """one launch on device copies; returns (n_eff, D, indices) on the host, `credit` (device, or None) is updated in place"""
    from hilcodec_amd import ops
    n = idx.shape[0]
    bits = vbr.bucket_bits(cfg, T, fec)
    dv = lambda t: None if t is None else t.to(DEV)
    d_idx = idx.to(DEV)
    n_eff, D = ops.vbr_select(z.to(DEV), d_idx, cb.to(DEV), min(n, vbr.floor_stages(cfg, fec)), cfg.rho, *bits, dv(n_b), dv(action),
                              dv(hold), credit)
    torch.cuda.synchronize()
    return n_eff.cpu(), D.cpu(), d_idx.cpu()


def compare(got, exp, what):
    for name, g, e in zip(("n_eff", "distortion", "indices"), got, exp):
        assert g.dtype == e.dtype and torch.equal(g, e), f"{what}: {name}"


@pytest.mark.parametrize("n", [1, 8, 12])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("B", [1, 5, 67])
def test_vbr_select_kernel_random(B, T, n):
    """random z, random (not arg-min) indices, some outside [0, K); per-slot ceilings, action and hold rows, a cap over consecutive
    hops; codebooks small enough that D wanders around D[0] and the rule fires at random stages"""
    gen = torch.Generator().manual_seed(B + 10 * T + 100 * n)
    cb = torch.randn(n + 1, K, C, generator=gen) * 0.05
    floor = min(2, n)
    capped = VbrConfig(0.01, n_min=floor, cap_kbps=0.75 * max(floor, (n + 1) // 2), burst_hops=3)
    plain = VbrConfig(0.01, n_min=floor)
    model = VbrModel(B, capped, n, T)
    credit = model.credit.clone().to(DEV)
    fired = set()
    for hop in range(5):
        z = torch.randn(B, T, C, generator=gen)
        idx = torch.randint(-1, K + 3, (n, B, T), generator=gen)
        n_b = torch.randint(0, n + 2, (B,), generator=gen, dtype=torch.int32)
        action = ((torch.rand(B, generator=gen) < 0.2) * torch.randint(-1, 3, (B,), generator=gen)).to(torch.int32)
        hold = (torch.rand(B, generator=gen) < 0.2).to(torch.int32) * torch.randint(1, 4, (B,), generator=gen, dtype=torch.int32)
        rows = (n_b, action, hold) if hop % 3 != 2 else (None, None, None)           # also without the optional rows
        exp = model.step(z, idx, cb, *rows)
        got = run_kernel(capped, z, idx, cb, *rows, credit, T)
        compare(got, exp, f"hop {hop}, capped")
        assert torch.equal(credit.cpu(), model.credit), f"hop {hop}: credit"
        exp = VbrModel(B, plain, n, T).step(z, idx, cb, *rows)
        compare(run_kernel(plain, z, idx, cb, *rows, None, T), exp, f"hop {hop}, no cap")
        fired |= set(exp[0].tolist())
    assert n == 1 or B == 1 or len(fired) >= 2


def constructed(gen, B, T, n, base, shift):
    """codebooks[s] = randn base^s; slot b = the sum of its first d_b codewords + 1e-3 randn, d_b cycling over 1..n; the indices past
    d_b are random"""
    cb = torch.stack([torch.randn(K, C, generator=gen) * base ** s for s in range(n)])
    idx = torch.randint(0, K, (n, B, T), generator=gen)
    d = torch.tensor([1 + (b + shift) % n for b in range(B)])
    z = 1e-3 * torch.randn(B, T, C, generator=gen)
    for s in range(n):
        z = z + torch.where((s < d)[:, None, None], cb[s][idx[s]], torch.zeros(()))
    return cb, idx, z, d


@pytest.mark.parametrize("n", [1, 8, 12])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("B", [1, 5, 67])
def test_vbr_select_kernel_constructed(B, T, n):
    gen = torch.Generator().manual_seed(7 + B + 10 * T + 100 * n)
    cfg = VbrConfig(20.0)
    part = max(1, n // 4)
    capped = VbrConfig(20.0, cap_kbps=0.75 * part, burst_hops=2)                   # a quarter of the stages per hop, a bucket of two hops
    model = VbrModel(B, capped, n, T)
    assert (model.rate_bits, model.burst_bits) == (10 * T * part, 20 * T * part)
    credit = model.credit.clone().to(DEV)
    cut = False
    for hop in range(4):
        cb, idx, z, d = constructed(gen, B, T, n, 0.9, hop)
        exp = VbrModel(B, cfg, n, T).step(z, idx, cb)
        assert exp[0].tolist() == d.tolist(), f"hop {hop}: the reference stops where the slot was built"
        compare(run_kernel(cfg, z, idx, cb, None, None, None, None, T), exp, f"hop {hop}")
        exp_c = model.step(z, idx, cb)                                             # the bucket state carries over the hops
        cut |= bool((exp_c[0] < exp[0]).any())
        compare(run_kernel(capped, z, idx, cb, None, None, None, credit, T), exp_c, f"hop {hop}, capped")
        assert torch.equal(credit.cpu(), model.credit), f"hop {hop}: credit"
        cb, idx, z, _ = constructed(gen, B, T, n, 0.5, hop)                         # magnitudes over 2^-11
        compare(run_kernel(cfg, z, idx, cb, None, None, None, None, T), VbrModel(B, cfg, n, T).step(z, idx, cb), f"hop {hop}, 2^-s")
    assert cut or n == 1 or B == 1                                                 # the cap did bind


def test_vbr_select_wide_latents_and_fec_floor():
    """C = 512 (8 channels per lane) and C = 64, the FEC floor, Nq > n"""
    gen = torch.Generator().manual_seed(5)
    B, T, n = 9, 2, 6
    for Cc in (64, 512):
        cb = torch.randn(n + 3, 16, Cc, generator=gen) * 0.05
        z = torch.randn(B, T, Cc, generator=gen)
        idx = torch.randint(0, 16, (n, B, T), generator=gen)
        cfg = VbrConfig(0.01, cap_kbps=6.0)
        m = VbrModel(B, cfg, n, T, fec_stages=3)
        credit = m.credit.clone().to(DEV)
        n_b = torch.tensor([6, 5, 4, 3, 2, 1, 6, 6, 6], dtype=torch.int32)
        exp = m.step(z, idx, cb, n_b)
        assert int(exp[0].min()) == 1 and int(exp[0][0]) >= 3
        compare(run_kernel(cfg, z, idx, cb, n_b, None, None, credit, T, fec=3), exp, f"C = {Cc}")
        assert torch.equal(credit.cpu(), m.credit)


@pytest.mark.parametrize("n", [15, 16, 17, 32])
def test_vbr_select_many_stages(n):
    """up to the most stages the kernel takes (32: D[0..32] sits in lanes 0..32), ceilings on both sides of 16"""
    gen = torch.Generator().manual_seed(n)
    B, T, Kc = 6, 2, 64
    cb = torch.randn(n, Kc, C, generator=gen) * 0.05
    cfg = VbrConfig(0.01, cap_kbps=0.75 * n, burst_hops=1)
    m = VbrModel(B, cfg, n, T)
    credit = m.credit.clone().to(DEV)
    for hop in range(2):
        z = torch.randn(B, T, C, generator=gen)
        idx = torch.randint(0, Kc, (n, B, T), generator=gen)
        n_b = torch.tensor([n, n - 1, 16, 1, n, 17], dtype=torch.int32)
        hold = torch.tensor([0, 0, 0, 0, hop, 0], dtype=torch.int32)
        exp = m.step(z, idx, cb, n_b, None, hold)
        compare(run_kernel(cfg, z, idx, cb, n_b, None, hold, credit, T), exp, f"hop {hop}")
        assert torch.equal(credit.cpu(), m.credit)
        # the rule is off (n_min = n_b): every stage of D is compared
        full = VbrConfig(0.01, n_min=n)
        compare(run_kernel(full, z, idx, cb, n_b, None, None, None, T), VbrModel(B, full, n, T).step(z, idx, cb, n_b), f"hop {hop}, all")


# ---------------------------------------------------------------- the sender
@pytest.fixture(scope="module")
def speech():
    """the streaming model with falling per-stage codebooks, scaled to its latents (module docstring)"""
    return vbr_speech_model()


class Eager:
    """the sender hop by hop without a graph: resample.reference -> the model's streaming encoder (fresh cache tensors, held slots put
    back, started slots zeroed) -> its quantiser -> VbrModel -> the wire packers (-> dtx.encode_model -> wire.pack_transport)"""

    def __init__(self, model, B, frames, n, cfg, sessions, input_rate=24000, fec=0, header=False, dtx_cfg=None):
        self.m, self.B, self.T, self.n, self.cfg = model, B, frames, n, cfg
        self.sessions, self.fec, self.header, self.dtx = sessions, fec, header, dtx_cfg
        x0 = torch.zeros(B, 1, HOP * frames, device=DEV)
        self.ce = [c.to(DEV) for c in model.initialize_cache(x0)[0]]
        self.rs = design(input_rate, 24000) if input_rate != 24000 else None
        self.hist = torch.zeros(B, 1, self.rs.history) if self.rs is not None else None
        self.vbr = VbrModel(B, cfg, n, frames, fec) if cfg is not None else None
        self.cb = model.quantizer._tables(DEV).codebooks.cpu()
        self.prev = [None] * B
        self.run = torch.zeros(B, dtype=torch.int32)
        self.ctr = [0] * B
        self.stride = wire.packet_bytes(n + fec, frames)

    def step(self, chunk, nb, fresh=(), held=()):
        """chunk [B, 1, S_in] on the device; nb: each slot's ceiling; fresh / held: the slots started / held on this hop"""
        B, T, n = self.B, self.T, self.n
        action = torch.zeros(B, dtype=torch.int32)
        hold = torch.zeros(B, dtype=torch.int32)
        if fresh:
            action[sorted(fresh)] = -1
        if held:
            hold[sorted(held)] = 1
        keep = hold.bool()
        x24 = chunk
        if self.rs is not None:
            self.hist[action != 0] = 0
            out, hist_new = reference(chunk, self.rs, self.hist)
            self.hist = torch.where(keep.view(B, 1, 1), self.hist, hist_new)
            x24 = out.to(DEV)
        with torch.no_grad():
            for c in self.ce:
                if fresh:
                    c[sorted(fresh)] = 0
            z, ce_new = self.m.encoder(x24.contiguous(), *self.ce)
            n_clip = torch.tensor(nb, dtype=torch.int32, device=DEV) if self.sessions else None
            idx = self.m.quantizer(z, n, n_clip=n_clip)
            self.ce = [torch.where(keep.to(DEV).view(B, 1, 1), old, new) for old, new in zip(self.ce, ce_new)]
        z, idx = z.cpu(), idx.cpu()
        rows = (torch.tensor(nb, dtype=torch.int32), action, hold) if self.sessions else (None, None, None)
        if self.vbr is not None:
            n_eff, D, idx = self.vbr.step(z, idx, self.cb, *rows)
        else:
            n_eff, D = torch.tensor(nb, dtype=torch.int32), None
        packets = torch.zeros(B, self.stride, dtype=torch.uint8)
        nbytes = torch.zeros(B, dtype=torch.int32)
        with_fec = [False] * B
        for b in range(B):
            if b in fresh:
                self.prev[b] = None
            if b in held:
                continue
            codes = idx[:int(n_eff[b]), b]
            blob = wire.pack_fec_packet(codes, self.prev[b]) if self.fec else wire.pack_stream_packet(codes)
            with_fec[b] = bool(self.fec) and self.prev[b] is not None
            packets[b, :len(blob)] = torch.frombuffer(bytearray(blob), dtype=torch.uint8)
            nbytes[b] = len(blob)
            if self.fec:
                self.prev[b] = idx[:self.fec, b].clone()
        idx = idx.clone()
        idx[:, keep] = -1
        kind = None
        if self.dtx is not None:
            self.run, kind, packets, nbytes, idx, _ = dtx.encode_model(x24.cpu().view(B, -1), self.run, action, hold, packets, nbytes,
                                                                       idx, None, self.dtx)
        if self.header:
            headed = torch.zeros(B, 3 + self.stride, dtype=torch.uint8)
            hbytes = torch.zeros(B, dtype=torch.int32)
            for b in range(B):
                c = 0 if b in fresh else self.ctr[b]
                self.ctr[b] = c if b in held else (c + 1) % 65536
                if b in held or int(nbytes[b]) == 0:
                    continue
                sid = kind is not None and int(kind[b]) == dtx.SID
                blob = wire.pack_transport(c, bytes(packets[b, :int(nbytes[b])].tolist()), int(n_eff[b]), sid=sid, fec=with_fec[b])
                headed[b, :len(blob)] = torch.frombuffer(bytearray(blob), dtype=torch.uint8)
                hbytes[b] = len(blob)
            packets, nbytes = headed, hbytes
        return packets, nbytes, idx, n_eff, D, kind


def signal(B, S_in, hops, seed, gaps=False):
    x = synth.synth_clips(B, S_in * hops, seed=seed)
    if not gaps:
        return x
    gain = torch.ones(B, hops)
    for b in range(0, B, 2):                                # every other stream falls silent for a few hops
        gain[b, 2 + b % 3:5 + b % 3] = 3e-5
    return (x.view(B, 1, hops, S_in) * gain.view(B, 1, hops, 1)).view(B, 1, hops * S_in)


def run_sender(model, B=8, frames=1, n=8, hops=7, seed=21, sessions=False, plan=False, input_rate=24000, fec=0, header=False,
               dtx_cfg=None, cap=True, distinct=3):
    from hilcodec_amd.graph_step import GraphedEncodeHop
    S_in = hop_samples(frames, input_rate)
    x = signal(B, S_in, hops, seed, gaps=dtx_cfg is not None).to(DEV)
    x0 = x[:, :, :S_in].contiguous()
    if input_rate != 24000:
        x0 = reference(x0, design(input_rate, 24000), None)[0].to(DEV)
    target = target_from_reference(model, B, frames, n, x0)
    # the cap: 6 of the 8 stages per hop, a bucket of two hops
    cfg = VbrConfig(target, cap_kbps=0.75 * max(1, (3 * n) // 4), burst_hops=2) if cap else VbrConfig(target)
    s = GraphedEncodeHop(model, B, HOP * frames, n, DEV, sessions=sessions, input_rate=input_rate, fec_stages=fec, header=header,
                         dtx=dtx_cfg, vbr=cfg)
    e = Eager(model, B, frames, n, cfg, sessions, input_rate, fec, header, dtx_cfg)
    assert s.n_eff.shape == (B,) and s.distortion.shape == (B, n + 1)
    if cap:
        assert torch.equal(s.credit.cpu(), e.vbr.credit)      # full buckets after the constructor's warm-up hops
    nb = [n] * B
    stopped = set()
    seen, kinds = set(), set()
    for h in range(hops):
        fresh, hold = set(), set()
        if plan and h == 2:
            s.start(1)
            s.start(3, n=5)
            fresh |= {1, 3}
            nb[1], nb[3] = n, 5
        if plan and h == 3:
            s.set_bitrate(2, 3)
            nb[2] = 3
            s.stop(6)
            stopped.add(6)
            hold.add(4)
        if plan and h == 4:
            s.start(5)                                      # started and held on the same hop
            fresh.add(5)
            hold |= {5, 4}
        if plan and h == 5:
            s.start(6, n=max(2, fec))
            stopped.discard(6)
            fresh.add(6)
            nb[6] = max(2, fec)
        chunk = x[:, :, S_in * h:S_in * (h + 1)].contiguous()
        pk, nbytes = s.step(chunk, hold=sorted(hold)) if sessions else s.step(chunk)
        held = hold | stopped
        exp_pk, exp_nb, exp_idx, exp_n, exp_D, exp_kind = e.step(chunk, nb, fresh, held)
        assert torch.equal(s.n_eff.cpu(), exp_n), f"hop {h}: n_eff"
        assert torch.equal(s.distortion.cpu(), exp_D), f"hop {h}: distortion"
        assert torch.equal(s.indices.cpu(), exp_idx), f"hop {h}: indices"
        assert torch.equal(nbytes.cpu(), exp_nb), f"hop {h}: nbytes"
        assert torch.equal(pk.cpu(), exp_pk), f"hop {h}: packets"
        if cap:
            assert torch.equal(s.credit.cpu(), e.vbr.credit), f"hop {h}: credit"
        if dtx_cfg is not None:
            assert torch.equal(s.kind.cpu(), exp_kind), f"hop {h}: kind"
            kinds |= set(exp_kind.tolist())
        free = [b for b in range(B) if b not in held and nb[b] == n]
        seen |= set(exp_n[free].tolist())                    # what the rule and the cap chose, not a ceiling or a hold
    assert len(seen) >= distinct, f"the reference's n_eff takes {sorted(seen)} only"
    if dtx_cfg is not None:
        assert dtx.SID in kinds and dtx.SPEECH in kinds
    return s, e


def test_sender_vbr(speech):
    run_sender(speech)


def test_sender_vbr_no_cap(speech):
    s, _ = run_sender(speech, cap=False, seed=22)
    with pytest.raises(RuntimeError, match="cap_kbps"):
        s.credit


def test_sender_vbr_sessions(speech):
    s, e = run_sender(speech, sessions=True, plan=True, hops=8, seed=23)
    # reset: every bucket full again, and the next hop matches a fresh reference
    s.reset()
    assert torch.equal(s.credit.cpu(), torch.full((8,), e.vbr.burst_bits, dtype=torch.int32))


def test_sender_vbr_fec_header(speech):
    run_sender(speech, sessions=True, plan=True, hops=8, seed=24, fec=2, header=True)


def test_sender_vbr_dtx(speech):
    run_sender(speech, sessions=True, hops=9, seed=25, dtx_cfg=dtx.DtxConfig(threshold_db=-50.0, hangover=1, sid_interval=2))


def test_sender_vbr_input_rate(speech):
    """16 kHz input: 320 samples at 24 kHz are not a whole number of samples at 16 kHz, so the hop is three frames (640 samples in)"""
    run_sender(speech, frames=3, hops=6, seed=26, input_rate=16000)


def test_vbr_none_is_inert(speech):
    from hilcodec_amd.graph_step import GraphedEncodeHop
    B, n, hops = 8, 8, 4
    x = signal(B, HOP, hops, 27).to(DEV)
    a = GraphedEncodeHop(speech, B, HOP, n, DEV, sessions=True, fec_stages=2, vbr=None)
    b = GraphedEncodeHop(speech, B, HOP, n, DEV, sessions=True, fec_stages=2)
    assert a.n_eff is None and a.distortion is None and len(a.outs[0]) == len(b.outs[0]) == 3
    for h in range(hops):
        chunk = x[:, :, HOP * h:HOP * (h + 1)].contiguous()
        pa, na = a.step(chunk, hold=[h % B])
        pb, nb = b.step(chunk, hold=[h % B])
        assert torch.equal(pa, pb) and torch.equal(na, nb) and torch.equal(a.indices, b.indices), h


def test_sender_checks(speech):
    from hilcodec_amd.graph_step import GraphedEncodeHop
    with pytest.raises(ValueError, match="header=True"):
        GraphedEncodeHop(speech, 2, HOP, 8, DEV, fec_stages=2, vbr=VbrConfig(20.0))
    with pytest.raises(ValueError, match="VbrConfig"):
        GraphedEncodeHop(speech, 2, HOP, 8, DEV, vbr=dtx.DtxConfig())
    with pytest.raises(ValueError, match="floor"):
        GraphedEncodeHop(speech, 2, HOP, 8, DEV, vbr=VbrConfig(20.0, n_min=3, cap_kbps=2.0))


# ---------------------------------------------------------------- through the unchanged receiver
def test_round_trip_through_the_receiver(speech):
    """headed VBR packets into play(), headerless ones into step(n_per_stream = wire.packet_n(nbytes, T)): both give the audio of a
    receiver fed wire-packed idx[:n_eff[b]] per slot"""
    from hilcodec_amd.graph_step import GraphedDecodeHop, GraphedEncodeHop
    B, n, T, hops, depth = 8, 8, 1, 8, 1
    x = signal(B, HOP, hops, 31).to(DEV)
    cfg = VbrConfig(target_from_reference(speech, B, T, n, x[:, :, :HOP].contiguous()), cap_kbps=4.5, burst_hops=2)
    tx = GraphedEncodeHop(speech, B, HOP, n, DEV, sessions=True, header=True, vbr=cfg)
    tp = GraphedEncodeHop(speech, B, HOP, n, DEV, sessions=True, vbr=cfg)
    jx = GraphedDecodeHop(speech, B, T, n, DEV, sessions=True, jitter=JitterConfig(depth=depth, capacity=4))
    ex = GraphedDecodeHop(speech, B, T, n, DEV, sessions=True)
    rf = GraphedDecodeHop(speech, B, T, n, DEV, sessions=True)
    played, stepped, ref, seen = [], [], [], set()
    for h in range(hops):
        chunk = x[:, :, HOP * h:HOP * (h + 1)].contiguous()
        pk, nb = tx.step(chunk)
        pp, nbp = tp.step(chunk)
        n_eff, idx = tx.n_eff.cpu(), tx.indices.cpu()
        assert torch.equal(tp.n_eff.cpu(), n_eff) and torch.equal(tp.indices.cpu(), idx)
        seen |= set(n_eff.tolist())
        played.append(jx.play(list(range(B)), pk.clone(), nb.cpu().tolist()).clone())
        stepped.append(ex.step(pp.clone(), [wire.packet_n(int(v), T) for v in nbp.cpu()]).clone())
        rows = torch.zeros(B, wire.packet_bytes(n, T), dtype=torch.uint8)
        for b in range(B):
            blob = wire.pack_stream_packet(idx[:int(n_eff[b]), b])
            rows[b, :len(blob)] = torch.frombuffer(bytearray(blob), dtype=torch.uint8)
        ref.append(rf.step(rows, n_eff.tolist()).clone())
    assert len(seen) >= 3, sorted(seen)
    for h in range(hops):
        assert torch.equal(stepped[h], ref[h]), f"hop {h}: step(packet_n)"
        assert bool(ref[h].any())
    for h in range(hops - depth):
        assert torch.equal(played[h + depth], ref[h]), f"hop {h}: play()"


# ---------------------------------------------------------------- production shape
def test_production_shape(speech):
    """1 024 streams, 3 hops, capped VBR, against VbrModel and the wire packers"""
    run_sender(speech, B=1024, hops=3, seed=41)
