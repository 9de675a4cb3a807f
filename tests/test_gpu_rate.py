"""GPU: report-driven rate control of the graphed sender (GraphedEncodeHop(rate=RateConfig(...))).  hilc_rate_ceiling and
hilc_rate_charge against rate.RateModel; the sender with a rate it never reaches against the sender without `rate`; scripted reports
against a sender driven with set_bitrate; answered NACKs charged; the closed loop of tests/rate_loop.py with the real sender and
receiver — every comparison bit for bit (torch.equal / np.array_equal)."""
import numpy as np
import pytest
import torch

from hilcodec_amd import dtx, jitter, rate, report, rtx, synth, wire
from hilcodec_amd.rate import RateConfig, RateModel
from hilcodec_amd.report import FecAdaptConfig, report_word
from hilcodec_amd.vbr import VbrConfig
from tests.hops import arrival_arrays, caches_equal
from tests.rate_loop import LOOP_JITTER, LOOP_RATE, LOOP_REPORT, Link, ReportLine, Trace, run_models

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
HOP = 320
N = 8
B_KERNEL = 70                                                # a last workgroup with two idle waves


@pytest.fixture(scope="module")
def speech():
    return synth.streaming_model()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


# ---------------------------------------------------------------- the kernels against RateModel
@pytest.mark.parametrize("m,T,header", [(0, 1, True), (2, 1, True), (2, 3, False)])
def test_rate_kernels(m, T, header):
    from hilcodec_amd import ops
    B, hops, P = B_KERNEL, 40, 2
    cfg = RateConfig(4.875 if T == 1 else 3.0, 24.0, 9.0, timeout_hops=6, burst_hops=3)       # 65 / 120 bits pay for the floors
    model = RateModel(B, cfg, N, T, m, header)
    rng = np.random.default_rng(100 * m + 10 * T + header)
    rows = torch.from_numpy(model.state.copy()).to(DEV)
    n_ceil = torch.full((B,), -9, dtype=torch.int32, device=DEV)
    tb = wire.transport_bytes(N, m, T)
    seq = rng.integers(0, 256, B)
    below = floor = 0
    for k in range(hops):
        words = np.zeros(B, dtype=np.int64)
        for b in np.nonzero(rng.random(B) < 0.2)[0]:
            how = rng.random()
            if how < 0.7:
                seq[b] = (seq[b] + int(rng.integers(1, 4))) & 255                # fresh
            elif how >= 0.85:
                seq[b] = (seq[b] - int(rng.integers(1, 100))) & 255              # older; in between: repeated
            words[b] = report_word(int(seq[b]), int(rng.choice([0, 3, 5, 6, 20, 25, 26, 27, 100, 255])), int(rng.integers(0, 256)))
        action = (rng.random(B) < 0.02).astype(np.int32) * rng.choice([-1, 1, 2], B).astype(np.int32)
        hold = (rng.random(B) < 0.15).astype(np.int32) * rng.choice([1, 2, 3], B).astype(np.int32)
        n_slot = rng.integers(max(m, 1), N + 1, B).astype(np.int32)
        prev = rng.integers(0, 1024, (B, 1 + m * T)).astype(np.int32)
        prev[:, 0] = rng.integers(0, 3, B)
        d_prev = dev(prev) if m else None
        want = model.ceiling(words, action, hold, n_slot, prev if m else None)
        ops.rate_ceiling(rows, n_ceil, N, T, m, header, cfg, report=dev(words), action=dev(action), hold=dev(hold), n_clip=dev(n_slot),
                         prev=d_prev)
        assert np.array_equal(rows.cpu().numpy(), model.state), k
        assert np.array_equal(n_ceil.cpu().numpy(), want), k
        assert d_prev is None or np.array_equal(d_prev.cpu().numpy(), prev), k           # read only
        below += int((want < n_slot).sum())
        # what the hop sent: nothing for a held slot, else anything up to the widest packet; a few answered NACKs, held or not
        nbytes = np.where(hold != 0, 0, rng.integers(0, tb + 1, B)).astype(np.int32)
        rtx_nbytes = (rng.integers(0, tb + 1, (B, P)) * (rng.random((B, P)) < 0.15)).astype(np.int32)
        if k % 7 == 3:
            rtx_nbytes[:] = 40 * tb                                              # more than any bucket holds: the debt floor
        model.charge(nbytes, rtx_nbytes)
        ops.rate_charge(dev(nbytes), rows, cfg, rtx_nbytes=dev(rtx_nbytes))
        assert np.array_equal(rows.cpu().numpy(), model.state), k
        floor += int((model.state[:, rate.RC_CREDIT] == -cfg.burst_hops * (model.state[:, rate.RC_RATE_Q8] >> 8)).sum())
    assert below > 0 and floor > 0
    assert all(model.state[:, rate.RC_REPORTS + i].sum() > 0 for i in range(len(rate.RC_NAMES)))
    # no report, action, hold, n or prev rows, no retransmissions: every slot ages, fills and reports what its credit pays for
    age = model.state[:, rate.RC_AGE].copy()
    want = model.ceiling()
    ops.rate_ceiling(rows, n_ceil, N, T, m, header, cfg)
    assert np.array_equal(rows.cpu().numpy(), model.state) and np.array_equal(n_ceil.cpu().numpy(), want)
    assert (model.state[:, rate.RC_AGE] != age).any()
    model.charge(nbytes)
    ops.rate_charge(dev(nbytes), rows, cfg)
    assert np.array_equal(rows.cpu().numpy(), model.state)


def test_kernels_refuse_bad_configs():
    """the library's error code reaches the caller and nothing is launched: the rows keep their sentinel"""
    z = lambda *s, v=0: torch.full(s, v, dtype=torch.int32, device=DEV)
    rows, n_ceil = z(2, rate.RC_WORDS, v=-9), z(2, v=-9)
    good = dict(frames=1, n=8, m=0, header=True, min_bits=35, max_bits=120, start_bits=120, high_q8=26, low_q8=5, increase_q8=13,
                burst_hops=8, timeout_hops=0)
    for kw in (dict(low_q8=26), dict(high_q8=256), dict(low_q8=-1), dict(increase_q8=-1), dict(burst_hops=0), dict(timeout_hops=-1),
               dict(min_bits=33), dict(m=2, min_bits=63), dict(start_bits=121), dict(start_bits=34), dict(n=33), dict(m=9),
               dict(max_bits=(1 << 22) + 1), dict(max_bits=1 << 22, burst_hops=257)):
        with pytest.raises(RuntimeError, match=r"hilc_rate_ceiling.*code -1"):
            torch.ops.hilcodec.rate_ceiling(None, None, None, None, None, rows, n_ceil, *{**good, **kw}.values())
    with pytest.raises(RuntimeError):
        torch.ops.hilcodec.rate_ceiling(None, None, None, None, None, z(2, rate.RC_WORDS - 1), n_ceil, *good.values())
    with pytest.raises(RuntimeError):
        torch.ops.hilcodec.rate_ceiling(None, None, None, z(3), None, rows, n_ceil, *good.values())
    with pytest.raises(RuntimeError):
        torch.ops.hilcodec.rate_ceiling(None, None, None, None, z(2, 4), rows, n_ceil, *{**good, "m": 2, "min_bits": 64}.values())
    for args in ((z(2), z(2, 5), rows, 8), (z(2), None, rows, 0)):
        with pytest.raises(RuntimeError, match=r"hilc_rate_charge.*code -1"):
            torch.ops.hilcodec.rate_charge(*args)
    with pytest.raises(RuntimeError):
        torch.ops.hilcodec.rate_charge(z(3), None, rows, 8)
    torch.cuda.synchronize()
    assert bool((rows == -9).all()) and bool((n_ceil == -9).all())


# ---------------------------------------------------------------- the sender graph
WIDE = RateConfig(4.875, 24.0)                               # 320 bits per hop: more than the widest packet of any variant below


@pytest.mark.parametrize("variant", ["plain", "fec_adapt", "vbr", "dtx_rtx"])
def test_sender_with_a_rate_it_never_reaches_is_the_sender_without(speech, variant):
    from hilcodec_amd.graph_step import GraphedEncodeHop
    B, hops = 3, 14
    kw = {"plain": dict(), "fec_adapt": dict(fec_stages=2, fec_adapt=FecAdaptConfig(calm_reports=1), header=True),
          "vbr": dict(vbr=VbrConfig(3.0, cap_kbps=6.0)), "dtx_rtx": dict(dtx=dtx.DtxConfig(), rtx=rtx.RtxConfig(), header=True)}[variant]
    tx = GraphedEncodeHop(speech, B, HOP, N, DEV, sessions=True, rate=WIDE, **kw)
    ref = GraphedEncodeHop(speech, B, HOP, N, DEV, sessions=True, **kw)
    x = synth.synth_clips(B, HOP * hops, seed=17).to(DEV)
    if variant == "dtx_rtx":
        x[1, :, HOP * 3:HOP * 11] = 0                         # SIDs and silence on slot 1
    for k in range(hops):
        if k == 5:
            tx.start(2)
            ref.start(2)
        if k == 8:
            tx.set_bitrate(0, 5)
            ref.set_bitrate(0, 5)
        holds = [0] if k in (6, 7) else []
        more, more_ref = {}, {}
        if variant == "fec_adapt" and k in (2, 9):             # the one report feeds hilc_fec_adapt of both; loss in the rule's dead zone
            more = more_ref = dict(reports=([1], [wire.pack_report(k, 0 if k == 2 else 20, 0)]))
        if variant == "dtx_rtx" and k in (4, 12):
            more = more_ref = dict(nacks=([0, 2], [wire.pack_nack(k - 3, 0b1), wire.pack_nack(k - 2, 0)]))
        xk = x[:, :, HOP * k:HOP * (k + 1)].contiguous()
        (pk, nb), (pk1, nb1) = tx.step(xk, hold=holds, **more), ref.step(xk, hold=holds, **more_ref)
        assert torch.equal(pk, pk1) and torch.equal(nb, nb1) and torch.equal(tx.indices, ref.indices), k
        assert caches_equal(tx.cache_enc, ref.cache_enc), k
        want = [5 if k >= 8 else N, N, N]
        assert tx.n_ceil.tolist() == want, k
        if variant == "fec_adapt":
            assert torch.equal(tx.fec_on, ref.fec_on) and torch.equal(tx.fec_adapt_state, ref.fec_adapt_state), k
        if variant == "vbr":
            assert torch.equal(tx.n_eff, ref.n_eff) and torch.equal(tx.credit, ref.credit) and torch.equal(tx.distortion, ref.distortion), k
        if variant == "dtx_rtx":
            assert torch.equal(tx.kind, ref.kind) and torch.equal(tx.rtx_packets, ref.rtx_packets), k
            assert torch.equal(tx.rtx_nbytes, ref.rtx_nbytes) and torch.equal(tx.rtx_state, ref.rtx_state), k
    st = tx.rate_state.cpu().numpy()
    assert not st[:, rate.RC_LIMITED].any() and not st[:, rate.RC_DECREASED].any() and (st[:, rate.RC_RATE_Q8] >= 320 * 256).all()
    # slot 0 was held on two hops, slot 1 heard its last report on hop 9 (fec_adapt), slot 2 started on hop 5
    assert st[:, rate.RC_AGE].tolist() == [hops - 2, hops - 9 if variant == "fec_adapt" else hops, hops - 5]
    if variant == "fec_adapt":
        assert st[1, rate.RC_REPORTS] == 2 and st[1, rate.RC_INCREASED] == 1
        assert tx.fec_adapt_state[1, report.FA_TURNED_OFF] == 1 and tx.fec_adapt_state[1, report.FA_TURNED_ON] == 1
    if variant == "dtx_rtx":
        assert int(tx.rtx_state[:, rtx.RX_SENT].sum()) >= 2 and bool((tx.kind == dtx.SPEECH).any())
    tx.reset()
    assert np.array_equal(tx.rate_state.cpu().numpy(), RateModel(B, WIDE, N, 1, kw.get("fec_stages", 0), kw.get("header", False)).state)
    assert tx.n_ceil.tolist() == [N] * B


SCRIPT = RateConfig(2.625, 9.0, burst_hops=2)                # a small bucket: the ceiling follows the rate within a few hops


def test_scripted_reports_lower_one_slot(speech):
    """0.5 reported loss on slot 1 only: its ceiling, byte count and header n fall as RateModel says, and its packets are those of a
    sender without `rate` whose set_bitrate was driven with the same n; slots 0 and 2 are those of a run without the reports"""
    from hilcodec_amd.graph_step import GraphedEncodeHop
    B, hops = 3, 36
    kw = dict(sessions=True, header=True)
    tx = GraphedEncodeHop(speech, B, HOP, N, DEV, rate=SCRIPT, **kw)
    quiet = GraphedEncodeHop(speech, B, HOP, N, DEV, rate=SCRIPT, **kw)
    driven = GraphedEncodeHop(speech, B, HOP, N, DEV, **kw)
    model = RateModel(B, SCRIPT, N, 1, 0, True)
    x = synth.synth_clips(B, HOP * hops, seed=23).to(DEV)
    seen = []
    for k in range(hops):
        words = np.zeros(B, dtype=np.int64)
        given = None
        if k % 3 == 1:
            words[1] = report_word(k, 128, 7)
            given = ([1], [wire.pack_report(k, 128, 7)])
        want = model.ceiling(words)
        driven.set_bitrate(1, int(want[1]))
        xk = x[:, :, HOP * k:HOP * (k + 1)].contiguous()
        pk, nb = tx.step(xk, reports=given)
        pq, nq = quiet.step(xk)
        pd, nd = driven.step(xk)
        assert np.array_equal(tx.n_ceil.cpu().numpy(), want), k
        model.charge(nb.cpu().numpy())
        assert np.array_equal(tx.rate_state.cpu().numpy(), model.state), k
        assert torch.equal(pk[1], pd[1]) and int(nb[1]) == int(nd[1]) == wire.TRANSPORT_HEADER + wire.packet_bytes(int(want[1]), 1), k
        assert int(pk[1, 2]) & wire.N_MASK == int(want[1]) and torch.equal(tx.indices[:, 1], driven.indices[:, 1]), k
        for b in (0, 2):
            assert torch.equal(pk[b], pq[b]) and int(nb[b]) == int(nq[b]) and torch.equal(tx.indices[:, b], quiet.indices[:, b]), (k, b)
            assert torch.equal(tx.rate_state[b], quiet.rate_state[b]) and int(tx.n_ceil[b]) == int(quiet.n_ceil[b]), (k, b)
        assert caches_equal(tx.cache_enc, quiet.cache_enc) and caches_equal(tx.cache_enc, driven.cache_enc), k
        seen.append(int(want[1]))
    assert seen[0] == N and min(seen) <= 2 and seen[-1] < seen[0] and model.state[1, rate.RC_DECREASED] == 12
    assert model.state[1, rate.RC_RATE_Q8] == 35 * 256 and rate.kbps(tx.rate_state[1], 1) == 2.625
    assert rate.kbps(tx.rate_state, 1).tolist() == [9.0, 2.625, 9.0]
    # a start refills the slot inside the graph; stop keeps the row
    tx.start(1)
    tx.stop(2)
    row2 = tx.rate_state[2].clone()
    pk, nb = tx.step(x[:, :, :HOP].contiguous())
    want = model.ceiling(action=[0, 1, 0], hold=[0, 0, 1])
    model.charge(nb.cpu().numpy())
    assert np.array_equal(tx.n_ceil.cpu().numpy(), want) and np.array_equal(tx.rate_state.cpu().numpy(), model.state)
    assert int(tx.n_ceil[1]) == N and tx.rate_state[1].tolist()[:2] == [120 * 256, 240 - 104] and torch.equal(tx.rate_state[2], row2)
    assert tx.rate_state[1, rate.RC_SEEN:].tolist() == [0, 0, 1, 0] + [0] * len(rate.RC_NAMES)        # the counters are cleared too


def test_answered_nacks_are_charged(speech):
    from hilcodec_amd.graph_step import GraphedEncodeHop
    B = 2
    kw = dict(sessions=True, header=True, rtx=rtx.RtxConfig(), rate=LOOP_RATE)
    tx, twin = GraphedEncodeHop(speech, B, HOP, N, DEV, **kw), GraphedEncodeHop(speech, B, HOP, N, DEV, **kw)
    x = synth.synth_clips(B, HOP * 6, seed=29).to(DEV)
    for k in range(6):
        xk = x[:, :, HOP * k:HOP * (k + 1)].contiguous()
        nacks = ([0], [wire.pack_nack(1, 0b1)]) if k == 4 else None          # hops 1 and 2 of slot 0
        holds = [0] if k == 4 else []                                      # a held slot still answers, and still pays
        pk, nb = tx.step(xk, hold=holds, nacks=nacks)
        twin.step(xk, hold=holds)
        again = tx.rtx_nbytes.cpu().numpy()
        diff = (twin.rate_state[:, rate.RC_CREDIT] - tx.rate_state[:, rate.RC_CREDIT]).tolist()
        if k < 4:
            assert not again.any() and diff == [0, 0], k
        elif k == 4:
            assert again[0].tolist() == [13, 13] and int(nb[0]) == 0 and diff == [8 * 26, 0]
        else:
            assert not again.any() and diff[0] > 0 and diff[1] == 0      # the next fill tops the twin up: slot 0 is still behind


# ---------------------------------------------------------------- end to end
def real_loop(speech, cap, hops, control):
    """tests/rate_loop.run_models with the real sender and receiver; returns (Trace, per hop the rate rows and n_ceil or None)"""
    from hilcodec_amd.graph_step import GraphedDecodeHop, GraphedEncodeHop
    B = 2
    tx = GraphedEncodeHop(speech, B, HOP, N, DEV, sessions=True, header=True, rate=LOOP_RATE if control else None)
    rx = GraphedDecodeHop(speech, B, 1, N, DEV, sessions=True, jitter=LOOP_JITTER, report=LOOP_REPORT, conceal=True)
    x = (torch.randn(B, 1, hops * HOP, generator=torch.Generator().manual_seed(9)) * 0.1).to(DEV)
    links, line, trace = [Link(cap) for _ in range(B)], ReportLine(), Trace(hops, B)
    rows = np.zeros((hops, B, rate.RC_WORDS), dtype=np.int32)
    ceil = np.zeros((hops, B), dtype=np.int32)
    delivered = np.zeros(B, dtype=np.int64)
    for t in range(hops):
        slots, blobs = line.reports_for(t)
        pk, nb = tx.step(x[:, :, HOP * t:HOP * (t + 1)].contiguous(), **(dict(reports=(slots, blobs) if slots else None) if control else {}))
        pk, nb = pk.cpu().numpy(), nb.cpu().numpy()
        if control:
            rows[t], ceil[t] = tx.rate_state.cpu().numpy(), tx.n_ceil.cpu().numpy()
        arrived = []
        for b in range(B):
            sent = pk[b, :nb[b]].tobytes()
            n_sent = sent[2] & wire.N_MASK
            assert not control or n_sent == ceil[t, b], (t, b)                  # the header's n is the sender's ceiling
            dropped, out = links[b].hop(sent)
            trace.n[t, b], trace.bits[t, b], trace.dropped[t, b] = n_sent, 8 * len(sent), dropped
            arrived += [(b, p) for p in out]
            delivered[b] += len(out)
        sl, packets, nbytes = arrival_arrays(arrived, rx.tstride)
        wav = rx.play(sl, torch.from_numpy(packets), nbytes)
        assert bool(torch.isfinite(wav).all()), t
        due, rep = rx.report_due.cpu().numpy(), rx.reports.cpu().numpy()
        line.push(t, [(b, rep[b].tobytes()) for b in range(B) if due[b]])
    js = rx.jitter_state.cpu().numpy()
    # the receiver took every packet that arrived: none malformed, late, early or twice
    assert js[:, jitter.STAT_ACCEPTED].tolist() == delivered.tolist()
    assert not js[:, [jitter.STAT_MALFORMED, jitter.STAT_LATE, jitter.STAT_EARLY, jitter.STAT_DUPLICATE]].any()
    assert (js[:, jitter.STAT_DECODED] >= delivered - 8).all()
    return trace, rows, ceil


def test_closed_loop_with_the_real_hops(speech):
    """GraphedEncodeHop(rate, header, sessions) -> a bottleneck of 60 bits per hop -> GraphedDecodeHop(jitter, report) -> reports back,
    400 hops: the sender's rate rows and ceilings are the model loop's on every hop, and the last 150 hops lose less than the same loop
    without `rate`"""
    hops, cap = 400, 60
    trace, rows, ceil = real_loop(speech, cap, hops, True)
    m_trace, _, m_rows, m_ceil = run_models(cap, hops=hops, B=2)
    assert np.array_equal(rows, m_rows) and np.array_equal(ceil, m_ceil)
    assert np.array_equal(trace.n, m_trace.n) and np.array_equal(trace.bits, m_trace.bits) and np.array_equal(trace.dropped, m_trace.dropped)
    trace0, _, _ = real_loop(speech, cap, hops, False)
    for b in range(2):
        with_, without = trace.loss(hops - 150, hops, b), trace0.loss(hops - 150, hops, b)
        print(f"slot {b}: loss over the last 150 hops {without:.3f} -> {with_:.3f}, {trace.mean_bits(hops - 150, hops, b):.1f} bits per hop")
        assert with_ < without and (trace0.n[:, b] == N).all()
    assert rows[-1, :, rate.RC_DECREASED].min() >= 1 and rows[-1, :, rate.RC_REPORTS].min() >= 20


# ---------------------------------------------------------------- accessors and constructor errors
def test_accessors_and_constructor_errors(speech):
    from hilcodec_amd.graph_step import GraphedEncodeHop
    with pytest.raises(ValueError, match="sessions"):
        GraphedEncodeHop(speech, 2, HOP, N, DEV, rate=LOOP_RATE)
    with pytest.raises(ValueError):
        GraphedEncodeHop(speech, 2, HOP, N, DEV, sessions=True, rate=FecAdaptConfig())
    with pytest.raises(ValueError, match="floor"):
        GraphedEncodeHop(speech, 2, HOP, N, DEV, sessions=True, header=True, fec_stages=2, rate=LOOP_RATE)      # 35 bits < 64
    x = torch.zeros(2, 1, HOP, device=DEV)
    plain = GraphedEncodeHop(speech, 2, HOP, N, DEV, sessions=True)
    for name in ("rate_state", "n_ceil"):
        with pytest.raises(RuntimeError):
            getattr(plain, name)
    with pytest.raises(RuntimeError):
        plain.step(x, reports=([0], [b"\x01\x00\x00"]))
    tx = GraphedEncodeHop(speech, 2, HOP, N, DEV, sessions=True, rate=RateConfig(2.625, 9.0, 6.0))
    assert tx.rate_state.shape == (2, rate.RC_WORDS) and tx.rate_state.dtype == torch.int32 and tx.rate_state.is_cuda
    assert tx.n_ceil.shape == (2,) and tx.n_ceil.dtype == torch.int32 and tx.n_ceil.tolist() == [N, N]
    assert tx.rate_state[:, :2].tolist() == [[80 * 256, 640]] * 2 and rate.kbps(tx.rate_state, 1).tolist() == [6.0, 6.0]
    for bad in (([2], [b"abc"]), ([0], [b"ab"]), ([0, 1], [b"abc"])):
        with pytest.raises(ValueError):
            tx.step(x, reports=bad)
    assert tx.rate_state[:, rate.RC_AGE].tolist() == [0, 0]                                             # nothing was launched
    # a slot named twice keeps its last report; a report applies to exactly one hop
    tx.step(x, reports=([1, 1], [wire.pack_report(5, 200, 0), wire.pack_report(9, 0, 0)]))
    st = tx.rate_state.cpu().numpy()
    assert st[1, rate.RC_LAST] == 9 and st[1, rate.RC_REPORTS] == 1 and st[:, rate.RC_INCREASED].tolist() == [0, 1]
    tx.step(x)
    st = tx.rate_state.cpu().numpy()
    assert st[1, rate.RC_REPORTS] == 1 and st[1, rate.RC_STALE] == 0 and st[:, rate.RC_AGE].tolist() == [2, 2]
