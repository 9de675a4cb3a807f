"""CPU: receiver reports and loss-adaptive FEC (hilcodec_amd/report.py, the definition of hilc_rx_report and hilc_fec_adapt): the wire
format of a report, both models by hand, the closed loop on the models (jitter.JitterModel as the receiver, a stand-in sender that
takes its FEC flag from FecAdaptModel) and the entry points.  Everything is integer: every comparison is exact."""
import numpy as np
import pytest
import torch

from hilcodec_amd import jitter, report, wire
from hilcodec_amd.report import FecAdaptConfig, FecAdaptModel, ReportConfig, ReportModel, report_word
from tests.hops import assert_entry_points
from tests.report_loop import LOOP, LOOP_ADAPT, check_closed_loop, closed_loop


# ---------------------------------------------------------------- wire
def test_report_round_trip_and_errors():
    assert wire.REPORT_BYTES == 3
    for fields in ((0, 0, 0), (1, 128, 64), (255, 255, 255), (17, 3, 250)):
        blob = wire.pack_report(*fields)
        assert isinstance(blob, bytes) and blob == bytes(fields) and wire.parse_report(blob) == fields
    assert wire.parse_report(np.array([9, 8, 7], dtype=np.uint8)) == (9, 8, 7)
    for bad in ((-1, 0, 0), (256, 0, 0), (0, 256, 0), (0, 0, -3), (0, 0, 1000), (1.5, 0, 0), (True, 0, 0)):
        with pytest.raises(ValueError):
            wire.pack_report(*bad)
    for bad in (b"", b"ab", b"abcd"):
        with pytest.raises(ValueError):
            wire.parse_report(bad)


def test_configs_check_their_ranges():
    assert ReportConfig() == ReportConfig(64, 16) and FecAdaptConfig() == FecAdaptConfig(8, 3, 4, 0, True)
    ReportConfig(8, 1), ReportConfig(256, 1024), FecAdaptConfig(on_q8=255, off_q8=0), FecAdaptConfig(on_q8=1, off_q8=0)
    for kw in (dict(window=7), dict(window=257), dict(interval=0), dict(interval=1025), dict(window=8.0), dict(interval=True)):
        with pytest.raises(ValueError):
            ReportConfig(**kw)
    for kw in (dict(on_q8=3, off_q8=3), dict(on_q8=2, off_q8=5), dict(on_q8=256), dict(off_q8=-1), dict(calm_reports=0),
               dict(timeout_hops=-1), dict(on_q8=8.0), dict(initial_on=1)):
        with pytest.raises(ValueError):
            FecAdaptConfig(**kw)
    assert report.RP_WORDS == report.RP_RING + 16 and len(report.RP_NAMES) == report.RP_RING
    assert report.FA_WORDS == report.FA_TIMEOUT + 1 and len(report.FA_NAMES) == report.FA_WORDS - report.FA_REPORTS


# ---------------------------------------------------------------- ReportModel by hand
STAT = {"D": jitter.STAT_DECODED, "F": jitter.STAT_FEC, "L": jitter.STAT_LOST, "N": jitter.STAT_NOISE}


class Feed:
    """one slot's jitter state row, moved one counter per hop"""

    def __init__(self, cfg):
        self.model = ReportModel(1, cfg)
        self.js = np.zeros((1, jitter.ST_WORDS), dtype=np.int32)

    def hop(self, cls=None, start=False):
        """cls: "D" / "F" / "L" / "N" or None (held, priming or grown); -> (report bytes, due)"""
        if start:
            self.js[:] = 0                                   # the jitter step clears its row on the same hop
        if cls is not None:
            self.js[0, STAT[cls]] += 1
        out = self.model.step(self.js, [int(start)])
        return tuple(int(v) for v in out["reports"][0]), int(out["due"][0])

    def run(self, classes):
        return [self.hop(c) for c in classes]


def test_report_model_by_hand():
    f = Feed(ReportConfig(8, 4))
    outs = f.run("DDFL")
    assert [o[1] for o in outs] == [0, 0, 0, 1] and outs[-1][0] == (1, 128, 64)
    assert all(o[0] == (0, 0, 0) for o in outs[:3])
    row = f.model.state[0]
    assert (row[report.RP_N], row[report.RP_F], row[report.RP_L], row[report.RP_HEAD], row[report.RP_PHASE]) == (4, 1, 1, 4, 0)
    assert row[report.RP_RING] == (report.CLASS_D | report.CLASS_D << 2 | report.CLASS_F << 4 | report.CLASS_L << 6)
    # a hop where no counter moved changes nothing: the row, the bytes; due is 0
    before = row.copy()
    assert f.hop(None) == ((1, 128, 64), 0) and np.array_equal(f.model.state[0], before)
    # entries 5..8: F L L L -> the window is D D F L F L L L: 6 of 8 missing, 4 lost
    outs = f.run("FLLL")
    assert outs[-1] == ((2, 192, 128), 1) and [o[1] for o in outs[:3]] == [0, 0, 0]
    assert row[report.RP_N] == 8 and row[report.RP_HEAD] == 0
    # the ninth entry pushes the first (a D) out of the counts, the tenth the second D, the eleventh the F
    f.hop("D")
    assert (row[report.RP_N], row[report.RP_F], row[report.RP_L]) == (8, 2, 4)
    f.hop("L")
    assert (row[report.RP_N], row[report.RP_F], row[report.RP_L]) == (8, 2, 5)
    f.hop("D")
    assert (row[report.RP_N], row[report.RP_F], row[report.RP_L]) == (8, 1, 5)
    # NOISE advances the interval but not N: the fourth classed hop since the last report is a noise hop and reports
    assert f.hop("N") == ((3, 192, 160), 1) and row[report.RP_N] == 8 and row[report.RP_HEAD] == 3
    assert row[report.RP_NOISE] == 1 and row[report.RP_REPORTS] == 3


def test_report_model_start_and_noise_only():
    f = Feed(ReportConfig(8, 4))
    f.run("DLDL")
    assert f.model.state[0, report.RP_SEQ] == 1 and f.model.reports[0].tolist() == [1, 128, 128]
    # a start clears the row, the bytes and the remembered counters; the next report is seq 1 again
    assert f.hop(None, start=True) == ((0, 0, 0), 0) and not f.model.state[0].any()
    assert f.run("DDDD")[-1] == ((1, 0, 0), 1)
    # a start on a hop that is classed (D = 0, depth 0): cleared first, then the hop enters the empty window
    assert f.hop("L", start=True) == ((0, 0, 0), 0)
    row = f.model.state[0]
    assert (row[report.RP_N], row[report.RP_L], row[report.RP_PHASE], row[report.RP_LOST]) == (1, 1, 1, 1)
    # R classed NOISE hops with N = 0 emit nothing, and the interval starts again
    g = Feed(ReportConfig(8, 4))
    assert all(o == ((0, 0, 0), 0) for o in g.run("NNNNNNNN"))
    assert g.model.state[0, report.RP_PHASE] == 0 and g.model.state[0, report.RP_SEQ] == 0
    assert g.run("NND")[-1] == ((0, 0, 0), 0) and g.hop("N") == ((1, 0, 0), 1)
    # the sequence number wraps mod 256
    h = Feed(ReportConfig(8, 1))
    outs = h.run("D" * 257)
    assert outs[0][0][0] == 1 and outs[254][0][0] == 255 and outs[255][0][0] == 0 and outs[256][0][0] == 1
    assert all(o[1] == 1 for o in outs)


def test_report_model_wide_ring():
    """W = 200: a ring of 13 words; the counts kept incrementally equal a recount of the last W entries"""
    W = 200
    f = Feed(ReportConfig(W, 16))
    rng = np.random.default_rng(3)
    entered = []
    for k in range(700):
        c = "DFLN"[int(rng.choice(4, p=[0.6, 0.15, 0.15, 0.1]))] if rng.random() < 0.9 else None
        f.hop(c)
        if c in ("D", "F", "L"):
            entered.append(c)
        row, last = f.model.state[0], entered[-W:]
        assert (row[report.RP_N], row[report.RP_F], row[report.RP_L]) == (len(last), last.count("F"), last.count("L")), k
    row = f.model.state[0]
    assert len(entered) > 2 * W and row[report.RP_RING:report.RP_RING + 13].all() and not row[report.RP_RING + 13:].any()
    if row[report.RP_REPORTS]:
        assert 0 < row[report.RP_LOSS] <= 255 and row[report.RP_RESIDUAL] <= row[report.RP_LOSS]
    # the ring itself holds the last W classes
    codes = {"D": report.CLASS_D, "F": report.CLASS_F, "L": report.CLASS_L}
    ring = [(int(row[report.RP_RING + i // 16]) >> 2 * (i % 16)) & 3 for i in range(W)]
    head = int(row[report.RP_HEAD])
    assert ring[head:] + ring[:head] == [codes[c] for c in entered[-W:]]


# ---------------------------------------------------------------- FecAdaptModel by hand
def words_of(B, **by_slot):
    w = np.zeros(B, dtype=np.int64)
    for slot, fields in by_slot.items():
        w[int(slot[1:])] = report_word(*fields)
    return w


def test_fec_adapt_on_and_off():
    cfg = FecAdaptConfig(on_q8=8, off_q8=3, calm_reports=3, initial_on=False)
    m = FecAdaptModel(1, cfg, 2)
    assert m.step().tolist() == [0]
    assert m.step(words_of(1, s0=(1, 7, 0))).tolist() == [0]           # in between: nothing
    assert m.step(words_of(1, s0=(2, 8, 1))).tolist() == [1]           # on at loss >= on_q8
    st = m.state[0]
    assert (st[report.FA_TURNED_ON], st[report.FA_LOSS], st[report.FA_RESIDUAL], st[report.FA_LAST]) == (1, 8, 1, 2)
    # off only after calm_reports consecutive calm reports; a report in between resets the count
    assert m.step(words_of(1, s0=(3, 3, 0))).tolist() == [1] and st[report.FA_CALM] == 1
    assert m.step(words_of(1, s0=(4, 0, 0))).tolist() == [1] and st[report.FA_CALM] == 2
    assert m.step(words_of(1, s0=(5, 5, 0))).tolist() == [1] and st[report.FA_CALM] == 0
    assert m.step(words_of(1, s0=(6, 3, 0))).tolist() == [1]
    assert m.step(words_of(1, s0=(7, 2, 0))).tolist() == [1]
    assert m.step().tolist() == [1]
    assert m.step(words_of(1, s0=(8, 1, 0))).tolist() == [0]
    assert (st[report.FA_TURNED_OFF], st[report.FA_TURNED_ON], st[report.FA_REPORTS], st[report.FA_STALE]) == (1, 1, 8, 0)
    # a loud report while on: no second TURNED_ON; calm reports while off: no second TURNED_OFF
    assert m.step(words_of(1, s0=(9, 0, 0))).tolist() == [0] and st[report.FA_TURNED_OFF] == 1
    assert m.step(words_of(1, s0=(10, 200, 9))).tolist() == [1] and m.step(words_of(1, s0=(11, 255, 9))).tolist() == [1]
    assert st[report.FA_TURNED_ON] == 2 and st[report.FA_CALM] == 0


def test_fec_adapt_sequence_numbers_and_timeout():
    cfg = FecAdaptConfig(calm_reports=1, timeout_hops=5)
    m = FecAdaptModel(1, cfg, 1)
    st = m.state[0]
    assert m.step(words_of(1, s0=(250, 0, 0))).tolist() == [0]         # any seq is accepted first
    before = st.copy()
    for seq in (250, 249, 122):                                          # a duplicate, an older one, d = 128
        m.state[0] = before
        m.step(words_of(1, s0=(seq, 200, 0)), hold=[1])
        want = before.copy()
        want[report.FA_STALE] += 1
        assert np.array_equal(st, want), seq
    m.state[0] = before
    assert m.step(words_of(1, s0=(3, 200, 0))).tolist() == [1]          # 250 -> 3 across the wrap: d = 9
    assert st[report.FA_LAST] == 3 and st[report.FA_AGE] == 1 and st[report.FA_REPORTS] == 2
    assert m.step(words_of(1, s0=(130, 0, 0))).tolist() == [0]          # d = 127: the last one accepted
    # a timeout restores initial_on and accepts any seq next
    for k in range(3):
        assert m.step().tolist() == [0] and st[report.FA_AGE] == 2 + k
    assert m.step().tolist() == [1]
    assert (st[report.FA_TIMEOUT], st[report.FA_SEEN], st[report.FA_AGE], st[report.FA_CALM]) == (1, 0, 0, 0)
    assert m.step(words_of(1, s0=(130, 0, 0))).tolist() == [0] and st[report.FA_STALE] == 0 and st[report.FA_SEEN] == 1
    # timeout_hops = 0: never
    n = FecAdaptModel(1, FecAdaptConfig(), 1)
    for _ in range(50):
        n.step()
    assert n.state[0, report.FA_AGE] == 50 and n.state[0, report.FA_TIMEOUT] == 0


def test_fec_adapt_hold_start_and_previous_codes():
    cfg = FecAdaptConfig(calm_reports=1, timeout_hops=4)
    B, mm, T = 3, 2, 3
    m = FecAdaptModel(B, cfg, mm, T)
    rng = np.random.default_rng(1)
    fresh = lambda: np.concatenate([np.ones((B, 1), np.int32), rng.integers(0, 1024, (B, mm * T)).astype(np.int32)], axis=1)
    # a held slot takes reports but does not age, and its previous-codes row is untouched; the others lose word 0 only
    prev = fresh()
    want = prev.copy()
    on = m.step(words_of(B, s0=(1, 0, 0), s1=(1, 0, 0), s2=(1, 9, 0)), hold=[1, 0, 0], prev=prev)
    assert on.tolist() == [0, 0, 1]
    want[1, 0] = 0
    assert np.array_equal(prev, want)
    assert m.state[:, report.FA_AGE].tolist() == [0, 1, 1] and m.state[:, report.FA_REPORTS].tolist() == [1, 1, 1]
    for _ in range(6):                                                   # ages 2, 3, 4 (timeout), 1, 2, 3; a held slot never ages
        m.step(hold=[1, 0, 0], prev=prev)
    assert m.state[:, report.FA_TIMEOUT].tolist() == [0, 1, 1] and m.state[:, report.FA_ON].tolist() == [0, 1, 1]
    # a start and a report on the same hop: clear first, then apply (the old sequence number is forgotten, the counters restart)
    m.step(words_of(B, s0=(9, 0, 0)))
    assert m.state[0, report.FA_STALE] == 0 and m.state[0, report.FA_REPORTS] == 2
    prev = fresh()
    on = m.step(words_of(B, s0=(9, 0, 0), s1=(77, 200, 3)), action=[1, -1, 0], hold=[0, 1, 0], prev=prev)
    assert on.tolist() == [0, 1, 1] and prev[:, 0].tolist() == [0, 1, 1]
    assert m.state[0].tolist() == [0, 1, 1, 9, 1, 0, 0, 1, 0, 0, 1, 0]
    assert m.state[1].tolist() == [1, 0, 1, 77, 0, 200, 3, 1, 0, 0, 0, 0]
    # initial_on = False: a cleared slot is off
    off = FecAdaptModel(2, FecAdaptConfig(initial_on=False), 1)
    assert off.state[:, report.FA_ON].tolist() == [0, 0] and off.step(action=[1, 0]).tolist() == [0, 0]


# ---------------------------------------------------------------- the closed loop


def standin_sender():
    """a sender in Python: random codes, the FEC flag from a FecAdaptModel of its own fed the same reports"""
    c = LOOP
    B, n, m, T = c["B"], c["n"], c["m"], c["T"]
    fm = FecAdaptModel(B, LOOP_ADAPT, m, T)
    rng = np.random.default_rng(12)
    tb = wire.transport_bytes(n, m, T)
    prev = np.zeros((B, 1 + m * T), dtype=np.int32)

    def send(k, slots, blobs, action):
        words = np.zeros(B, dtype=np.int64)
        for s, blob in zip(slots, blobs):
            words[s] = report_word(*wire.parse_report(blob))
        prev[np.asarray(action) != 0] = 0
        fm.step(words, action, prev=prev)
        packets, nbytes = np.zeros((B, tb), dtype=np.uint8), []
        for b in range(B):
            codes = rng.integers(0, 1024, (n, T))
            fec = bool(prev[b, 0])
            body = np.concatenate([codes, prev[b, 1:].reshape(m, T)]) if fec else codes
            blob = wire.pack_transport(k, wire.pack_stream_packet(torch.from_numpy(body)), n, fec=fec)
            packets[b, :len(blob)] = np.frombuffer(blob, dtype=np.uint8)
            nbytes.append(len(blob))
            prev[b, 0], prev[b, 1:] = 1, codes[:m].reshape(-1)
        return packets, nbytes

    return send


def test_closed_loop_on_the_models():
    hist, jm, rm, fm = closed_loop(standin_sender())
    switches = check_closed_loop(hist, jm, fm)
    # the exact hops, from the models: the first report is due on the 8th played hop (hop 9, D = 2), arrives at hop 12, and the third
    # calm one at hop 28; the first loss (hop 61) shows in the report of hop 65, which arrives at hop 68
    assert switches == {0: (28,), 1: (28,), 2: (28, 68, 228), 3: (28, 68, 228)}
    assert jm.state[2:, jitter.STAT_LOST].tolist() == [1, 1] and jm.state[2:, jitter.STAT_FEC].tolist() == [14, 14]
    wide = wire.transport_bytes(LOOP["n"], LOOP["m"], LOOP["T"])
    assert (hist["nbytes"][1:, 0] == wide).sum() == 27                   # redundant sections out of 299 packets on a clean slot
    assert rm.state[:, report.RP_REPORTS].tolist() == [37] * 4


# ---------------------------------------------------------------- entry points
def test_report_entry_points():
    assert_entry_points(["hilc_rx_report", "hilc_fec_adapt"], in_abi16_line=True)
