"""The closed loop of receiver reports and loss-adaptive FEC on the models (no tests here): jitter.JitterModel as the receiver,
report.ReportModel reporting, report.FecAdaptModel deciding; the sender is the caller's.  tests/test_report_cpu.py closes it with a
stand-in sender in Python, tests/test_gpu_report.py with the graphed hops."""
import numpy as np

from hilcodec_amd import jitter, report, wire
from hilcodec_amd.jitter import JitterConfig, JitterModel
from hilcodec_amd.report import FecAdaptConfig, FecAdaptModel, ReportConfig, ReportModel, report_word

LOOP = dict(B=4, n=8, m=2, T=1, D=2, C=8, hops=300, K=8, delay=3)


LOOP_REPORT, LOOP_ADAPT = ReportConfig(32, 8), FecAdaptConfig(calm_reports=3)


def lost_in_loop(k, b):
    return b >= 2 and 60 <= k < 180 and k % 8 == 5


def closed_loop(send, observe=None):
    """the loop of the issue on the models: each hop the sender takes the reports that became due `delay` hops ago (`send(k, slots,
    blobs, action) -> (packets uint8 [B, tbytes], nbytes [B])`), slots 2-3 lose every packet with k % 8 == 5 in [60, 180), the rest
    arrives on its hop; JitterModel plays, ReportModel reports.  `observe(k, slots, packets, nbytes, action, jm, rm, fm)` sees every
    hop.  Returns the per-hop history and the models."""
    c = LOOP
    B = c["B"]
    jm = JitterModel(B, JitterConfig(c["D"], c["C"]), c["n"], c["m"], c["T"], c["K"], True)
    rm = ReportModel(B, LOOP_REPORT)
    fm = FecAdaptModel(B, LOOP_ADAPT, c["m"], c["T"])
    tb = wire.transport_bytes(c["n"], c["m"], c["T"])
    flight, hist = [], dict(on=[], nbytes=[], lost=[], fec=[], due=[])
    for k in range(c["hops"]):
        action = np.full(B, int(k == 0), dtype=np.int32)
        now = [f for f in flight if f[0] == k]
        flight = [f for f in flight if f[0] != k]
        slots, blobs = [f[1] for f in now], [f[2] for f in now]
        words = np.zeros(B, dtype=np.int64)
        for s, blob in zip(slots, blobs):
            words[s] = report_word(*wire.parse_report(blob))
        on = fm.step(words, action)
        packets, nbytes = send(k, slots, blobs, action)
        packets, nbytes = np.asarray(packets, dtype=np.uint8).reshape(B, tb), [int(v) for v in nbytes]
        arrive = [b for b in range(B) if not lost_in_loop(k, b)]
        args = (arrive, packets[arrive], [nbytes[b] for b in arrive])
        jm.step(action, np.zeros(B, dtype=np.int32), *args)
        out = rm.step(jm.state, action)
        for b in np.nonzero(out["due"])[0]:
            flight.append((k + c["delay"], int(b), bytes(out["reports"][b])))
        for key, v in (("on", on), ("nbytes", nbytes), ("lost", jm.state[:, jitter.STAT_LOST].copy()),
                       ("fec", jm.state[:, jitter.STAT_FEC].copy()), ("due", out["due"])):
            hist[key].append(np.asarray(v).copy())
        if observe is not None:
            observe(k, *args, action, jm, rm, fm)
    return {key: np.stack(v) for key, v in hist.items()}, jm, rm, fm


def check_closed_loop(hist, jm, fm):
    """the relations the issue requires, on the history of either loop; -> the hops of the switches, for the record"""
    c = LOOP
    plain, wide = wire.transport_bytes(c["n"], 0, c["T"]), wire.transport_bytes(c["n"], c["m"], c["T"])
    on, nbytes, lost = hist["on"], hist["nbytes"], hist["lost"]
    fa = fm.state
    switches = {}
    for b in (0, 1):
        assert fa[b, report.FA_TURNED_OFF] == 1 and fa[b, report.FA_TURNED_ON] == 0
        off = int(np.nonzero(on[:, b] == 0)[0][0])
        assert (on[off:, b] == 0).all() and (nbytes[off:, b] == plain).all()    # no redundant section after the switch-off
        assert (nbytes[1:off, b] == wide).all() and nbytes[0, b] == plain
        assert jm.state[b, jitter.STAT_LOST] == 0 and jm.state[b, jitter.STAT_FEC] == 0
        switches[b] = (off,)
    for b in (2, 3):
        assert fa[b, report.FA_TURNED_ON] == 1 and fa[b, report.FA_TURNED_OFF] == 2
        off = int(np.nonzero(on[:, b] == 0)[0][0])
        again = off + int(np.nonzero(on[off:, b] == 1)[0][0])
        off2 = again + int(np.nonzero(on[again:, b] == 0)[0][0])
        assert (on[off:again, b] == 0).all() and (on[again:off2, b] == 1).all() and (on[off2:, b] == 0).all()
        # STAT_LOST stops growing once fec_on is 1 (a packet lost before the switch-on is still played, as lost, D hops later)
        assert (lost[again + c["D"]:, b] == lost[again + c["D"], b]).all()
        before = sum(lost_in_loop(k, b) for k in range(again))
        assert jm.state[b, jitter.STAT_FEC] + jm.state[b, jitter.STAT_LOST] == 15
        assert jm.state[b, jitter.STAT_LOST] <= before + 1
        # every loss from the switch-on hop on is repaired
        after = sum(lost_in_loop(k, b) for k in range(again, c["hops"]))
        assert jm.state[b, jitter.STAT_FEC] >= after
        assert (nbytes[again:off2, b] == wide).all() and (nbytes[off2:, b] == plain).all()
        switches[b] = (off, again, off2)
    assert (fa[:, report.FA_STALE] == 0).all() and (fa[:, report.FA_TIMEOUT] == 0).all()
    return switches
