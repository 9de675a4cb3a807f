"""GPU: receiver reports and loss-adaptive FEC of the graphed hops (GraphedDecodeHop(report=ReportConfig(...)),
GraphedEncodeHop(fec_adapt=FecAdaptConfig(...))).  hilc_rx_report and hilc_fec_adapt against report.py's models; the adaptive sender
against a sender with FEC and one without; the reporting receiver against the receiver without reports; the closed loop of
tests/test_report_cpu.py with the real sender and receiver — every comparison bit for bit (torch.equal / np.array_equal)."""
import numpy as np
import pytest
import torch

from hilcodec_amd import dtx, jitter, report, synth, wire
from hilcodec_amd.jitter import AdaptConfig, JitterConfig, JitterModel
from hilcodec_amd.report import FecAdaptConfig, FecAdaptModel, ReportConfig, ReportModel, report_word
from hilcodec_amd.vbr import VbrConfig
from tests.hops import Network, caches_equal
from tests.report_loop import LOOP, LOOP_ADAPT, LOOP_REPORT, check_closed_loop, closed_loop

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
HOP = 320
ADAPT = AdaptConfig(window=8, resync=3, force_windows=2)
B_KERNEL = 70                                                # a last workgroup with two idle waves


@pytest.fixture(scope="module")
def speech():
    return synth.streaming_model()


# ---------------------------------------------------------------- hilc_rx_report against ReportModel
@pytest.fixture(scope="module")
def state_trace():
    """150 hops of jitter state rows of 70 slots: JitterModel on Network traffic with FEC, DTX, holds and starts; computed once"""
    B, n, m, K, T, hops = B_KERNEL, 8, 2, 8, 1, 150
    cfg = JitterConfig(2, 8, adapt=ADAPT)
    model = JitterModel(B, cfg, n, m, T, K, True)
    net = Network(B, n, m, K, T, seed=2, loss=0.1, delay=3, dup=0.02, hold=0.03, start=0.004, sid=0.05, mild=False)
    trace = []
    for _ in range(hops):
        slots, packets, nbytes, action, hold = net.hop()
        model.step(action, hold, slots, packets, nbytes)
        trace.append((model.state.copy(), action.copy()))
    st = model.state
    assert all(st[:, i].sum() > 0 for i in (jitter.STAT_DECODED, jitter.STAT_FEC, jitter.STAT_LOST, jitter.STAT_NOISE))
    assert model.adapt[:, jitter.AD_GROWN].sum() > 0                              # hops without a class besides held ones
    return trace


@pytest.mark.parametrize("W,R", [(8, 4), (64, 16), (200, 1)])
def test_rx_report_kernel(state_trace, W, R):
    from hilcodec_amd import ops
    B, cfg = B_KERNEL, ReportConfig(W, R)
    model = ReportModel(B, cfg)
    rows = torch.zeros(B, report.RP_WORDS, dtype=torch.int32, device=DEV)
    blobs = torch.zeros(B, 3, dtype=torch.uint8, device=DEV)
    due = torch.full((B,), -9, dtype=torch.int32, device=DEV)
    classes, start_on_window = set(), 0
    for k, (js, action) in enumerate(state_trace):
        before = model.state.copy()
        start_on_window += int(((action != 0) & (before[:, report.RP_N] > 0)).sum())
        want = model.step(js, action)
        d_js = torch.from_numpy(js).to(DEV)
        ops.rx_report(d_js, rows, blobs, due, cfg, action=torch.from_numpy(action).to(DEV))
        assert np.array_equal(rows.cpu().numpy(), model.state), k
        assert np.array_equal(blobs.cpu().numpy(), want["reports"]), k
        assert np.array_equal(due.cpu().numpy(), want["due"]), k
        assert np.array_equal(d_js.cpu().numpy(), js), k                          # read-only
        for i, c in ((report.RP_DECODED, "D"), (report.RP_FEC, "F"), (report.RP_LOST, "L"), (report.RP_NOISE, "N")):
            if (model.state[:, i] != np.where(action != 0, 0, before[:, i])).any():
                classes.add(c)
    assert classes == set("DFLN") and start_on_window >= 1
    assert (model.state[:, report.RP_REPORTS] > 0).sum() >= B // 2
    # without an action row no slot is cleared
    ops.rx_report(d_js, rows, blobs, due, cfg)
    model.step(js, np.zeros(B, dtype=np.int32))
    assert np.array_equal(rows.cpu().numpy(), model.state) and not due.any()


def test_kernels_refuse_bad_configs():
    from hilcodec_amd import ops

    class Cfg:
        def __init__(self, w, r):
            self.window, self.interval = w, r

    z = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt, device=DEV)
    args = (z(2, jitter.ST_WORDS), z(2, report.RP_WORDS), z(2, 3, dt=torch.uint8), z(2))
    for w, r in ((7, 4), (257, 4), (8, 0), (8, 1025)):
        with pytest.raises(RuntimeError, match="hilc_rx_report"):
            ops.rx_report(*args, Cfg(w, r))
    with pytest.raises(RuntimeError):
        ops.rx_report(z(2, 13), *args[1:], ReportConfig())
    fa = (z(2, 3), z(2, report.FA_WORDS), z(2), 2, 1)

    class Fa:
        on_q8, off_q8, calm_reports, timeout_hops, initial_on = 8, 3, 4, 0, True

    for name, v in (("on_q8", 3), ("on_q8", 256), ("off_q8", -1), ("calm_reports", 0), ("timeout_hops", -1)):
        bad = Fa()
        setattr(bad, name, v)
        with pytest.raises(RuntimeError, match="hilc_fec_adapt"):
            ops.fec_adapt(*fa, bad)
    with pytest.raises(RuntimeError):
        ops.fec_adapt(z(2, 4), *fa[1:], Fa())


# ---------------------------------------------------------------- hilc_fec_adapt against FecAdaptModel
@pytest.mark.parametrize("m,T", [(1, 1), (2, 3)])
def test_fec_adapt_kernel(m, T):
    from hilcodec_amd import ops
    B, hops = B_KERNEL, 120
    cfg = FecAdaptConfig(on_q8=8, off_q8=3, calm_reports=2, timeout_hops=12, initial_on=bool(m == 1))
    model = FecAdaptModel(B, cfg, m, T)
    rng = np.random.default_rng(10 * m + T)
    rows = torch.from_numpy(model.state.copy()).to(DEV)
    fec_on = torch.full((B,), -9, dtype=torch.int32, device=DEV)
    seq = rng.integers(0, 256, B)
    untouched = 0
    for k in range(hops):
        words = np.zeros(B, dtype=np.int64)
        for b in np.nonzero(rng.random(B) < 0.2)[0]:
            how = rng.random()
            if how < 0.7:
                seq[b] = (seq[b] + int(rng.integers(1, 4))) & 255                # fresh
            elif how < 0.85:
                pass                                                             # repeated
            else:
                seq[b] = (seq[b] - int(rng.integers(1, 100))) & 255              # older
            words[b] = report_word(int(seq[b]), int(rng.choice([0, 2, 3, 4, 7, 8, 9, 60, 255])), int(rng.integers(0, 256)))
        action = (rng.random(B) < 0.01).astype(np.int32) * rng.choice([-1, 1, 2], B).astype(np.int32)
        hold = (rng.random(B) < 0.15).astype(np.int32) * rng.choice([1, 2, 3], B).astype(np.int32)
        prev = rng.integers(0, 1024, (B, 1 + m * T)).astype(np.int32)
        prev[:, 0] = rng.integers(0, 3, B)
        d_prev = torch.from_numpy(prev).to(DEV)
        given = prev.copy()
        on = model.step(words, action, hold, prev=prev)
        ops.fec_adapt(d_prev, rows, fec_on, m, T, cfg, report=torch.from_numpy(words.astype(np.int32)).to(DEV),
                      action=torch.from_numpy(action).to(DEV), hold=torch.from_numpy(hold).to(DEV))
        assert np.array_equal(rows.cpu().numpy(), model.state), k
        assert np.array_equal(fec_on.cpu().numpy(), on), k
        assert np.array_equal(d_prev.cpu().numpy(), prev), k
        # only word 0 of the slots that are off and not held changes
        changed = given != prev
        assert not changed[:, 1:].any() and not changed[(hold != 0) | (on == 1), 0].any(), k
        untouched += int(((hold != 0) & (on == 0) & (given[:, 0] != 0)).sum())
    assert untouched > 0
    assert all(model.state[:, report.FA_REPORTS + i].sum() > 0 for i in range(len(report.FA_NAMES)))
    # no report, action or hold rows: every slot ages
    age = model.state[:, report.FA_AGE].copy()
    model.step()
    ops.fec_adapt(d_prev, rows, fec_on, m, T, cfg)
    assert np.array_equal(rows.cpu().numpy(), model.state) and (model.state[:, report.FA_AGE] != age).any()


# ---------------------------------------------------------------- the sender graph
SENDER_ADAPT = FecAdaptConfig(on_q8=8, off_q8=3, calm_reports=2, timeout_hops=9)


def sender_script(k):
    """hop k of the sender test: (reports {slot: (seq, loss, residual)}, starts, holds, bitrates {slot: n})"""
    reports, starts, holds, rates = {}, [], [], {}
    if k in (3, 5):
        reports[0] = (k, 0, 0)                               # slot 0: off at hop 5 ...
    if k == 12:
        reports[0] = (k, 40, 9)                              # ... on again at 12 (the packet of hop 12 carries hop 11's codes)
    if k in (2, 4):
        reports[1] = (k, 3, 0)                               # slot 1: off at hop 4, then silence: on again by timeout at hop 13
    # slot 2 never hears anything: on throughout, timeouts only
    if k % 3 == 0:
        reports[3] = (k, 1, 0)                               # slot 3: calm throughout: off from hop 3, a start at 20, off again at 24
    if k == 20:
        starts.append(3)
    if k % 4 == 1:
        reports[4] = (200 + k // 2 if k % 8 == 1 else 150, 0 if k < 25 else 99, 1)      # slot 4: fresh and stale reports, some while held
    if k in (9, 10, 17, 30):
        holds.append(4)
    if k in (6, 7):
        holds.append(0)                                      # held while off: the row keeps its previous codes
    if k == 8:
        rates[0], rates[4] = 2, 3
    if k == 15:
        rates[0] = 4
    if k == 26:
        starts.append(1)
        holds.append(1)                                      # a start on a held hop
    return reports, starts, holds, rates


@pytest.mark.parametrize("variant", ["header", "plain", "dtx", "vbr"])
def test_adaptive_sender_against_fec_and_no_fec(speech, variant):
    from hilcodec_amd.graph_step import GraphedEncodeHop
    B, n, m, hops = 5, 4, 2, 40
    kw = dict(sessions=True, header=variant != "plain")
    if variant == "dtx":
        kw["dtx"] = dtx.DtxConfig(order=4)                   # the defaults but for the order: a SID of 1 + K bytes must fit n = 4's 5-byte row
    if variant == "vbr":
        kw["vbr"] = VbrConfig(3.0, n_min=m)                  # the floor of the sender without FEC is the FEC senders' max(n_min, m)
    tx = GraphedEncodeHop(speech, B, HOP, n, DEV, fec_stages=m, fec_adapt=SENDER_ADAPT, **kw)
    tx_on = GraphedEncodeHop(speech, B, HOP, n, DEV, fec_stages=m, **kw)
    tx_off = GraphedEncodeHop(speech, B, HOP, n, DEV, fec_stages=0, **kw)
    model = FecAdaptModel(B, SENDER_ADAPT, m, 1)
    x = synth.synth_clips(B, HOP * hops, seed=31).to(DEV)
    if variant == "dtx":
        x[1, :, HOP * 14:HOP * 24] = 0                        # a silent stretch: SIDs and silence on slot 1
        x[3, :, HOP * 5:] *= 1e-5
    narrow = wire.transport_bytes(n, 0, 1) if kw["header"] else wire.packet_bytes(n, 1)
    switched_on = 0
    for k in range(hops):
        reports, starts, holds, rates = sender_script(k)
        action, hold = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        for s in (tx, tx_on, tx_off):
            for b in starts:
                s.start(b)
            for b, v in rates.items():
                s.set_bitrate(b, v)
        action[starts], hold[holds] = 1, 1
        words = np.zeros(B, dtype=np.int64)
        for b, fields in reports.items():
            words[b] = report_word(*fields)
        was_on = model.state[:, report.FA_ON].copy()
        on = model.step(words, action, hold)
        xk = x[:, :, HOP * k:HOP * (k + 1)].contiguous()
        slots = list(reports)
        blobs = [wire.pack_report(*reports[b]) for b in slots]
        given = (slots, blobs) if k % 2 else (torch.tensor(slots), torch.tensor([list(r) for r in blobs], dtype=torch.uint8).reshape(-1, 3))
        pk, nb = tx.step(xk, hold=holds, reports=given if slots else None)
        pk1, nb1 = tx_on.step(xk, hold=holds)
        pk0, nb0 = tx_off.step(xk, hold=holds)
        assert np.array_equal(tx.fec_on.cpu().numpy(), on) and np.array_equal(tx.fec_adapt_state.cpu().numpy(), model.state), k
        if k == 8 and variant != "dtx":
            assert int(nb0[0]) > 0 and int(nb1[0]) > 0       # held on hops 6 and 7 with nothing else to upload on 7: released on 8
        pk, pk1, pk0 = pk.cpu(), pk1.cpu(), pk0.cpu()
        wide0 = torch.zeros_like(pk1)
        wide0[:, :narrow] = pk0
        for b in range(B):
            want_pk, want_nb = (pk1[b], nb1[b]) if on[b] else (wide0[b], nb0[b])
            assert torch.equal(pk[b], want_pk) and int(nb[b]) == int(want_nb), (k, b)
            if on[b] and not was_on[b] and not hold[b] and not action[b]:
                switched_on += int(nb1[b]) > int(nb0[b])     # the first packet after switching back on carries the previous hop's codes
        assert torch.equal(tx.indices, tx_on.indices) and torch.equal(tx.indices, tx_off.indices), k
        assert caches_equal(tx.cache_enc, tx_on.cache_enc) and caches_equal(tx.cache_enc, tx_off.cache_enc), k
        if variant == "dtx":
            assert torch.equal(tx.kind, tx_on.kind) and torch.equal(tx.kind, tx_off.kind), k
        if variant == "vbr":
            assert torch.equal(tx.n_eff, tx_on.n_eff) and torch.equal(tx.n_eff, tx_off.n_eff), k
    st = model.state
    assert switched_on >= 1
    assert st[0, report.FA_TURNED_OFF] == 1 and st[0, report.FA_TURNED_ON] == 1 and st[3, report.FA_TURNED_OFF] == 1
    assert st[4, report.FA_STALE] > 0 and st[0, report.FA_TIMEOUT] >= 1 and st[2, report.FA_TIMEOUT] >= 1
    # reset clears every row to its initial state
    tx.reset()
    fresh = FecAdaptModel(B, SENDER_ADAPT, m, 1)
    assert np.array_equal(tx.fec_adapt_state.cpu().numpy(), fresh.state) and bool((tx.fec_on == 1).all())


def test_adaptive_sender_without_reports_is_the_fec_sender(speech):
    from hilcodec_amd.graph_step import GraphedEncodeHop
    B, n, m, hops = 3, 4, 2, 12
    kw = dict(sessions=True, fec_stages=m, header=True)
    tx = GraphedEncodeHop(speech, B, HOP, n, DEV, fec_adapt=FecAdaptConfig(), **kw)
    tx_on = GraphedEncodeHop(speech, B, HOP, n, DEV, **kw)
    x = synth.synth_clips(B, HOP * hops, seed=5).to(DEV)
    for k in range(hops):
        if k == 4:
            tx.start(1)
            tx_on.start(1)
        holds = [2] if k in (6, 7) else []
        xk = x[:, :, HOP * k:HOP * (k + 1)].contiguous()
        (pk, nb), (pk1, nb1) = tx.step(xk, hold=holds), tx_on.step(xk, hold=holds)
        assert torch.equal(pk, pk1) and torch.equal(nb, nb1) and torch.equal(tx.indices, tx_on.indices), k
        assert caches_equal(tx.cache_enc, tx_on.cache_enc) and torch.equal(tx.hop_index, tx_on.hop_index), k
        assert bool((tx.fec_on == 1).all())
    assert tx.fec_adapt_state[:, report.FA_AGE].tolist() == [hops, hops - 4, hops - 2]


# ---------------------------------------------------------------- the receiver graph
def test_reporting_receiver_only_observes(speech):
    from hilcodec_amd.graph_step import GraphedDecodeHop
    B, n, m, K, hops = 6, 8, 2, 8, 80
    cfg, rcfg = JitterConfig(2, 8, adapt=ADAPT), ReportConfig(8, 4)
    kw = dict(sessions=True, conceal=True, fec_stages=m, cng_order=K, jitter=cfg)
    rx = GraphedDecodeHop(speech, B, 1, n, DEV, report=rcfg, **kw)
    ref = GraphedDecodeHop(speech, B, 1, n, DEV, **kw)
    jm, rm = JitterModel(B, cfg, n, m, 1, K, True), ReportModel(B, rcfg)
    net = Network(B, n, m, K, 1, seed=4, loss=0.08, delay=6, dup=0.02, bad=0.02, hold=0.03, sid=0.06, restart=0.01, every=10)
    for k in range(hops):
        slots, packets, nbytes, action, hold = net.hop()
        if k == 50:
            assert rm.state[2, report.RP_N] > 0
            action[2] = 1                                    # a start in the middle clears the slot's report row
        for b in np.nonzero(action)[0]:
            rx.start(int(b))
            ref.start(int(b))
        jm.step(action, hold, slots, packets, nbytes)
        want = rm.step(jm.state, action)
        held = np.nonzero(hold)[0].tolist()
        a = rx.play(slots, torch.from_numpy(packets), nbytes, hold=held).clone()
        b = ref.play(slots, torch.from_numpy(packets), nbytes, hold=held).clone()
        assert torch.equal(a, b), k
        assert caches_equal(rx.cache_dec, ref.cache_dec), k
        for name in ("jitter_state", "jitter_adapt", "concealed", "cng_state"):
            assert torch.equal(getattr(rx, name), getattr(ref, name)), (name, k)
        assert np.array_equal(rx.jitter_state.cpu().numpy(), jm.state), k
        assert np.array_equal(rx.reports.cpu().numpy(), want["reports"]), k
        assert np.array_equal(rx.report_due.cpu().numpy(), want["due"]), k
        assert np.array_equal(rx.report_state.cpu().numpy(), rm.state), k
    assert (rm.state[:, report.RP_REPORTS] > 0).all() and rm.state[:, report.RP_F].sum() + rm.state[:, report.RP_L].sum() > 0
    # a start of every slot with no arrival on that hop: every report row, report and flag is zero
    assert rx.report_state.any() and rx.reports.any()
    for b in range(B):
        rx.start(b)
    rx.play([], torch.zeros(0, rx.tstride, dtype=torch.uint8), [])
    assert not rx.report_state.any() and not rx.reports.any() and not rx.report_due.any()


# ---------------------------------------------------------------- end to end
def test_closed_loop_with_the_real_hops(speech):
    """the closed loop of tests/test_report_cpu.py with the real sender and receiver.  From the models (and equal to the CPU loop):
    every slot switches off at hop 28; the lossy slots switch on at 68 and off again at 228, with 1 hop lost and 14 repaired."""
    from hilcodec_amd.graph_step import GraphedDecodeHop, GraphedEncodeHop
    c = LOOP
    B, n, m, hops = c["B"], c["n"], c["m"], c["hops"]
    tx = GraphedEncodeHop(speech, B, HOP, n, DEV, sessions=True, fec_stages=m, header=True, fec_adapt=LOOP_ADAPT)
    rx = GraphedDecodeHop(speech, B, 1, n, DEV, sessions=True, jitter=JitterConfig(c["D"], c["C"]), report=LOOP_REPORT, conceal=True,
                          fec_stages=m, cng_order=c["K"])
    x = (torch.randn(B, 1, hops * HOP, generator=torch.Generator().manual_seed(9)) * 0.1).to(DEV)

    def send(k, slots, blobs, action):
        for b in np.nonzero(action)[0]:
            tx.start(int(b))
            rx.start(int(b))
        pk, nb = tx.step(x[:, :, HOP * k:HOP * (k + 1)].contiguous(), reports=(slots, blobs) if slots else None)
        return pk.cpu().numpy(), nb.cpu().numpy().tolist()

    def observe(k, slots, packets, nbytes, action, jm, rm, fm):
        rx.play(slots, torch.from_numpy(np.ascontiguousarray(packets)), nbytes)
        assert np.array_equal(tx.fec_on.cpu().numpy(), fm.state[:, report.FA_ON]), k
        assert np.array_equal(tx.fec_adapt_state.cpu().numpy(), fm.state), k
        assert np.array_equal(rx.jitter_state.cpu().numpy(), jm.state), k
        assert np.array_equal(rx.reports.cpu().numpy(), rm.reports), k
        assert np.array_equal(rx.report_due.cpu().numpy(), rm.due), k
        assert np.array_equal(rx.report_state.cpu().numpy(), rm.state), k

    hist, jm, rm, fm = closed_loop(send, observe)
    switches = check_closed_loop(hist, jm, fm)
    assert switches == {0: (28,), 1: (28,), 2: (28, 68, 228), 3: (28, 68, 228)}
    plain = wire.transport_bytes(n, 0, 1)
    assert (hist["nbytes"][28:, :2] == plain).all()          # the bytes sent after the switch-off, per hop


# ---------------------------------------------------------------- accessors and constructor errors
def test_accessors_and_constructor_errors(speech):
    from hilcodec_amd.graph_step import GraphedDecodeHop, GraphedEncodeHop
    jc = JitterConfig(2, 8)
    with pytest.raises(ValueError):
        GraphedDecodeHop(speech, 2, 1, 8, DEV, sessions=True, report=ReportConfig())                  # needs jitter
    with pytest.raises(ValueError):
        GraphedDecodeHop(speech, 2, 1, 8, DEV, sessions=True, jitter=jc, report=FecAdaptConfig())
    plain = GraphedDecodeHop(speech, 2, 1, 8, DEV, sessions=True, jitter=jc)
    for name in ("reports", "report_due", "report_state"):
        with pytest.raises(RuntimeError):
            getattr(plain, name)
    rx = GraphedDecodeHop(speech, 2, 1, 8, DEV, sessions=True, jitter=jc, report=ReportConfig())
    assert rx.reports.shape == (2, 3) and rx.reports.dtype == torch.uint8 and rx.reports.is_cuda
    assert rx.report_due.shape == (2,) and rx.report_due.dtype == torch.int32
    assert rx.report_state.shape == (2, report.RP_WORDS) and rx.report_state.dtype == torch.int32

    cfg = FecAdaptConfig()
    with pytest.raises(ValueError):
        GraphedEncodeHop(speech, 2, HOP, 8, DEV, fec_stages=2, fec_adapt=cfg)                          # needs sessions
    with pytest.raises(ValueError):
        GraphedEncodeHop(speech, 2, HOP, 8, DEV, sessions=True, fec_adapt=cfg)                         # needs fec_stages >= 1
    with pytest.raises(ValueError):
        GraphedEncodeHop(speech, 2, HOP, 8, DEV, sessions=True, fec_stages=2, fec_adapt=ReportConfig())
    x = torch.zeros(2, 1, HOP, device=DEV)
    fixed = GraphedEncodeHop(speech, 2, HOP, 8, DEV, sessions=True, fec_stages=2)
    for name in ("fec_on", "fec_adapt_state"):
        with pytest.raises(RuntimeError):
            getattr(fixed, name)
    with pytest.raises(RuntimeError):
        fixed.step(x, reports=([0], [b"\x01\x00\x00"]))
    tx = GraphedEncodeHop(speech, 2, HOP, 8, DEV, sessions=True, fec_stages=2, fec_adapt=FecAdaptConfig(calm_reports=1))
    assert tx.fec_on.shape == (2,) and tx.fec_on.dtype == torch.int32 and tx.fec_on.tolist() == [1, 1]
    assert tx.fec_adapt_state.shape == (2, report.FA_WORDS) and tx.fec_adapt_state.dtype == torch.int32
    for bad in (([2], [b"abc"]), ([-1], [b"abc"]), ([0], [b"ab"]), ([0], [b"abcd"]), ([0, 1], [b"abc"]),
                ([0], torch.zeros(1, 4, dtype=torch.uint8)), ([0], torch.zeros(1, 3, dtype=torch.int32))):
        with pytest.raises(ValueError):
            tx.step(x, reports=bad)
    assert tx.fec_adapt_state[:, report.FA_AGE].tolist() == [0, 0]                                      # nothing was launched
    # a slot named twice keeps its last report; a report applies to exactly one hop
    tx.step(x, reports=([1, 1], [wire.pack_report(5, 200, 0), wire.pack_report(9, 0, 0)]))
    st = tx.fec_adapt_state.cpu().numpy()
    assert st[1, report.FA_LAST] == 9 and st[1, report.FA_REPORTS] == 1 and tx.fec_on.tolist() == [1, 0]
    tx.step(x)
    st = tx.fec_adapt_state.cpu().numpy()
    assert st[1, report.FA_REPORTS] == 1 and st[1, report.FA_STALE] == 0 and st[:, report.FA_AGE].tolist() == [2, 2]
    # a step that raises before its upload (a wrong input shape) drops its reports: the next hop does not apply them
    with pytest.raises(RuntimeError):
        tx.step(torch.zeros(2, 1, HOP + 1, device=DEV), reports=([0], [wire.pack_report(1, 0, 0)]))
    tx.step(x)
    st = tx.fec_adapt_state.cpu().numpy()
    assert st[:, report.FA_REPORTS].tolist() == [0, 1] and st[:, report.FA_AGE].tolist() == [3, 3] and tx.fec_on.tolist() == [1, 0]


def test_slot_held_two_hops_in_a_row_is_released(speech):
    """a slot held on two hops in a row with nothing else to upload on the second advances on the third: the sender and the loopback
    hop against twins whose second hop has an upload of its own (a bitrate for another slot)"""
    from hilcodec_amd.graph_step import GraphedEncodeHop, GraphedHop
    B, n = 3, 4
    x = synth.synth_clips(B, HOP * 5, seed=8).to(DEV)
    a, b = (GraphedEncodeHop(speech, B, HOP, n, DEV, sessions=True) for _ in range(2))
    la, lb = (GraphedHop(speech, B, HOP, n, DEV, sessions=True) for _ in range(2))
    for k in range(5):
        xk = x[:, :, HOP * k:HOP * (k + 1)].contiguous()
        holds = [1] if k in (1, 2) else []
        if k == 2:
            b.set_bitrate(0, n)                              # no change of slot 0's n, but an upload on this hop
            lb.set_bitrate(0, n)
        (pa, na), (pb, nb) = a.step(xk, hold=holds), b.step(xk, hold=holds)
        assert torch.equal(pa, pb) and torch.equal(na, nb) and torch.equal(a.indices, b.indices), k
        assert caches_equal(a.cache_enc, b.cache_enc), k
        assert na.tolist() == [wire.packet_bytes(n, 1), 0 if holds else wire.packet_bytes(n, 1), wire.packet_bytes(n, 1)], k
        (ia, wa), (ib, wb) = la.step(xk, hold=holds), lb.step(xk, hold=holds)
        assert torch.equal(ia, ib) and torch.equal(wa, wb), k
        assert bool((ia[:, 1] == -1).all()) == bool(holds), k
