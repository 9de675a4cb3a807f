"""CPU: the selective forwarding hop's definition (hilcodec_amd/forward.py, the definition of hilc_forward_classify and
hilc_forward_route): the row layouts against the header, the configuration, the trim rule stated twice (in `wire` functions and in
bits), the selection and route rules on scripted rooms, and the invariants and the independence of rooms under random traffic
(tests/forward_loop.py).  Everything is integer: every comparison is exact."""
import itertools
import os
import re

import numpy as np
import pytest
import torch

from hilcodec_amd import forward, wire
from hilcodec_amd.forward import ForwardConfig, ForwardModel, trim_bits, trim_packet
from tests.forward_loop import Membership, Traffic, check_hop, malformed, random_packet, random_sid
from tests.hops import HEADER, assert_entry_points


# ---------------------------------------------------------------- layouts, entry points, configuration
def test_layouts_match_header():
    """forward.<NAME> is `#define HILC_FORWARD_<NAME>`, value for value, in both directions, and both rows are dense"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    env, header = {}, {}
    for name, expr in re.findall(r"^#define (HILC_\w+)[ \t]+(\S.*?)[ \t]*$", text, re.M):
        env[name] = eval(re.sub(r"\b(0x[0-9A-Fa-f]+|\d+)[uU]\b", r"\1", expr), {"__builtins__": {}}, env)
        if name.startswith("HILC_FORWARD_"):
            header[name[len("HILC_FORWARD_"):]] = env[name]
    python = {k: v for k, v in vars(forward).items() if k.isupper() and not k.startswith("_") and isinstance(v, int) and not isinstance(v, bool)}
    assert len(header) >= 16 and header == python
    for pre, width, names in (("SD_", "SD_WORDS", forward.SD_NAMES), ("LR_", "LR_WORDS", forward.LR_NAMES)):
        words = sorted(v for k, v in header.items() if k.startswith(pre) and k != width)
        assert words == list(range(header[width])) and len(names) == header[width], pre
    assert (forward.MAX_FANOUT, forward.MAX_BURST) == (8, 4)


def test_entry_points_are_declared_exported_and_bound():
    assert_entry_points(("hilc_forward_classify", "hilc_forward_route"), in_abi16_line=True)
    assert os.path.isfile(os.path.join(os.path.dirname(forward.__file__), "csrc", "forward.hip"))
    import hilcodec_amd
    assert hilcodec_amd.forward is forward and hilcodec_amd.ForwardConfig is ForwardConfig
    assert hilcodec_amd.GraphedForwardHop.__name__ == "GraphedForwardHop"


def test_config_checks_its_ranges():
    assert ForwardConfig() == ForwardConfig(3, 2, 8, True)
    ForwardConfig(1, 1, 0, False), ForwardConfig(8, 4, 255, True)
    for kw in (dict(fanout=0), dict(fanout=9), dict(burst=0), dict(burst=5), dict(hang_hops=-1), dict(hang_hops=256), dict(fanout=3.0),
               dict(burst=True), dict(hang_hops="8"), dict(keep_fec=1), dict(keep_fec=None)):
        with pytest.raises(ValueError):
            ForwardConfig(**kw)
    for bad in (dict(batch=0), dict(n=0), dict(n=32), dict(T=0), dict(m=5), dict(n=20, m=13)):
        kw = dict(batch=2, n=4, T=1, m=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            ForwardModel(kw["batch"], ForwardConfig(), kw["n"], kw["T"], kw["m"])


# ---------------------------------------------------------------- the trim rule, stated twice
N_MAX, K_SID = 8, 4
TRIM_CASES = [(T, m, n, fec) for T in (1, 2, 3) for m in (0, 2) for n in range(1, N_MAX + 1) for fec in ((False, True) if m and n >= m else (False,))]


def padded(blob, tb):
    row = np.zeros(tb, dtype=np.uint8)
    row[:len(blob)] = np.frombuffer(blob, dtype=np.uint8)
    return row


@pytest.fixture(scope="module")
def trim_sources():
    """per case: the headed packet with random pad bits and its codes"""
    rng = np.random.default_rng(3)
    return {case: random_packet(rng, int(rng.integers(0, 65536)), case[2], case[0], case[1], case[3]) for case in TRIM_CASES}


@pytest.mark.parametrize("T", (1, 2, 3))
def test_trim_packet(trim_sources, T):
    """every packet n, every L, FEC present or not, keep_fec both ways: the cut parses, its primary codes are the source's first
    min(n, L) stages, its redundant codes the source's or absent exactly when the rule says so, its length follows, it is canonical
    whatever the input's pad bits, and the bit-window statement (trim_bits) gives the same bytes"""
    cuts = set()
    for (T_, m, n, fec), (packet, codes) in trim_sources.items():
        if T_ != T:
            continue
        tb = wire.transport_bytes(N_MAX, m, T)
        hop = (packet[0] << 8) | packet[1]
        for L, keep_fec in itertools.product(range(1, N_MAX + 1), (False, True)):
            got = trim_packet(padded(packet, tb), len(packet), L, T, N_MAX, m, K_SID, keep_fec)
            keep = min(n, L)
            red = fec and keep_fec and keep >= m
            assert isinstance(got, bytes) and len(got) == 3 + wire.packet_bytes(keep + (m if red else 0), T)
            h2, sid2, fec2, n2, body2 = wire.parse_transport(got, len(got), T, N_MAX, m, K_SID)
            assert (h2, sid2, fec2, n2) == (hop, False, red, keep)
            out_codes = wire.unpack_stream_packet(body2, keep + (m if red else 0), T)
            assert torch.equal(out_codes[:keep], codes[:keep])
            assert not red or torch.equal(out_codes[keep:], codes[n:])
            # canonical: the bytes of the packet made from the codes alone, so the pad bits are zero
            assert got == wire.pack_transport(hop, wire.pack_fec_packet(codes[:keep], codes[n:] if red else None), keep, fec=red)
            if keep == n and red == fec:
                clean = wire.pack_transport(hop, wire.pack_stream_packet(codes), n, fec=fec)
                assert got == clean and (got != packet or packet == clean)
            bits, length = trim_bits(np.frombuffer(packet, dtype=np.uint8), L, T, m, keep_fec)
            assert length == len(got) and bits.tobytes() == got, (T, m, n, fec, L, keep_fec)
            cuts.add((10 * keep * T) % 8)
    assert cuts == {(10 * k * T) % 8 for k in range(1, N_MAX + 1)} and (T != 1 or cuts == {0, 2, 4, 6})      # T = 1 alone: every offset
    assert T != 1 or any(p != wire.pack_transport((p[0] << 8) | p[1], wire.pack_stream_packet(c), case[2], fec=case[3])
                         for case, (p, c) in trim_sources.items() if case[0] == 1)       # some input did carry pad bits


def test_trim_packet_sid_and_malformed():
    rng = np.random.default_rng(4)
    for T, m in itertools.product((1, 2, 3), (0, 2)):
        tb = wire.transport_bytes(N_MAX, m, T)
        sid = random_sid(rng, 77, K_SID)
        for L, keep_fec in itertools.product((1, 5, 8), (False, True)):
            assert trim_packet(padded(sid, tb), len(sid), L, T, N_MAX, m, K_SID, keep_fec) == sid
            bits, length = trim_bits(np.frombuffer(sid, dtype=np.uint8), L, T, m, keep_fec)
            assert bits.tobytes() == sid and length == len(sid)
        with pytest.raises(ValueError):
            trim_packet(padded(sid, tb), len(sid), 4, T, N_MAX, m, None, True)       # a SID without comfort noise
        good = random_packet(rng, 5, 4, T, m, False)[0]
        seen = set()
        for _ in range(60):
            bad, nb = malformed(rng, good, N_MAX, T, m)
            seen.add((len(bad), nb, bad[2] if len(bad) > 2 else -1))
            with pytest.raises(ValueError):
                trim_packet(padded(bad, tb), nb, 4, T, N_MAX, m, K_SID, True)
        assert len(seen) >= 5
        with pytest.raises(ValueError):
            trim_packet(padded(good, tb), len(good), 0, T, N_MAX, m, K_SID, True)
    # the FEC flag on a packet with n < m, and on a receiver without FEC
    p = bytearray(random_packet(rng, 5, 1, 1, 2, False)[0])
    p[2] |= wire.FEC_BIT
    for m in (0, 2):
        with pytest.raises(ValueError):
            trim_packet(bytes(p), len(p), 4, 1, N_MAX, m, K_SID, True)


# ---------------------------------------------------------------- scripted rooms
class Script:
    """a ForwardModel driven by hand: hop(sends, events) with sends = {slot: "c" codes / "f" codes with FEC / "s" SID / "x" malformed,
    one letter per arrival}"""

    def __init__(self, B, cfg, n=4, T=1, m=0, K=K_SID):
        self.B, self.cfg, self.n, self.T, self.m, self.K = B, cfg, n, T, m, K
        self.model, self.mem = ForwardModel(B, cfg, n, T, m, K), Membership(B, n)
        self.rng, self.h = np.random.default_rng(9), 0
        self.tb = self.model.tb

    def hop(self, sends=None, events=()):
        self.mem.apply(events)
        slots, blobs = [], []
        for b, kinds in (sends or {}).items():
            for kind in kinds:
                good = random_packet(self.rng, self.h, self.n, self.T, self.m, kind == "f")[0]
                blob = {"c": good, "f": good, "s": random_sid(self.rng, self.h, self.K)}.get(kind) or malformed(self.rng, good, self.n, self.T, self.m)
                slots.append(b)
                blobs.append(blob if isinstance(blob, tuple) else (blob, len(blob)))
        self.h += 1
        packets = np.stack([padded(p, self.tb) for p, _ in blobs]) if blobs else np.zeros((0, self.tb), dtype=np.uint8)
        self.sent = {(b, i): blobs[a][0] for b in set(slots) for i, a in enumerate(a for a, s in enumerate(slots) if s == b)}
        self.res = self.model.step(slots, packets, [nb for _, nb in blobs], self.mem.room, self.mem.layers, self.mem.action())
        return self.res

    def routes(self, b):
        return self.res["routes"][b].tolist()

    def row(self, b, j, k=0):
        nb = int(self.res["out_nbytes"][b, j, k])
        return self.res["out"][b, j, k, :nb].tobytes()

    def canon(self, b, i, L=None):
        """what slot b's i-th arrival of the last hop is forwarded as at L layers (default: all): the pad bits zero"""
        p = self.sent[b, i]
        return trim_packet(p, len(p), self.n if L is None else L, self.T, self.n, self.m, self.K, self.cfg.keep_fec)

    def sender(self, b, name):
        return int(self.model.sender.state[b, forward.SD_NAMES.index(name)])

    def listener(self, b, name):
        return int(self.model.listener.state[b, forward.LR_NAMES.index(name)])


def join_all(B, rooms):
    return [("join", b, rooms[b]) for b in range(B) if rooms[b] >= 0]


def test_selection_never_routes_self_or_another_room():
    s = Script(6, ForwardConfig(fanout=3))
    s.hop({b: "c" for b in range(6)}, join_all(6, [0, 0, 0, 1, 1, -1]))
    assert s.routes(0) == [1, 2, -1] and s.routes(1) == [0, 2, -1] and s.routes(2) == [0, 1, -1]
    assert s.routes(3) == [4, -1, -1] and s.routes(4) == [3, -1, -1] and s.routes(5) == [-1, -1, -1]
    assert s.sender(5, "codes") == 1 and s.sender(5, "hang") == 9          # a slot without a room is classified like any other
    assert s.res["new_routes"][0].tolist() == [1, 1, 0] and s.listener(0, "switches") == 2
    assert s.row(0, 0) == s.sent[1, 0] and s.row(0, 1) == s.sent[2, 0] and s.row(3, 0) == s.sent[4, 0]
    assert not s.res["out_nbytes"][5].any() and not s.res["out"][5].any()
    assert s.listener(0, "packets") == 2 and s.listener(0, "bytes") == len(s.sent[1, 0]) + len(s.sent[2, 0])


def test_incumbent_keeps_its_route_and_a_newcomer_takes_the_lowest_free_one():
    s = Script(6, ForwardConfig(fanout=3, hang_hops=1))
    s.hop({2: "c", 4: "c"}, join_all(6, [0] * 6))
    assert s.routes(0) == [2, 4, -1]
    s.hop({4: "c", 1: "c"})                                  # 2 hangs over, 1 is new: it takes the lowest free route
    assert s.routes(0) == [2, 4, 1] and s.res["new_routes"][0].tolist() == [0, 0, 1]
    s.hop({4: "c", 1: "c"})                                  # 2 has been quiet for hang_hops + 1 hops: evicted
    assert s.routes(0) == [-1, 4, 1] and not s.res["new_routes"][0].any() and s.sender(2, "hang") == 0 and s.sender(2, "since") == 0
    s.hop({4: "c", 1: "c", 5: "c", 3: "c"})                  # 3 and 5 are new, one route is free: ties break by slot
    assert s.routes(0) == [3, 4, 1] and s.res["new_routes"][0].tolist() == [1, 0, 0]
    s.hop({4: "c", 5: "c", 3: "c"})                          # 1 hangs over with SD_HANG 1, three others have 2: 5 takes its route
    assert s.routes(0) == [3, 4, 5] and s.res["new_routes"][0].tolist() == [0, 0, 1]
    s.hop({5: "c", 3: "c"})                                  # 4 hangs over and nobody else is active: it keeps its index
    assert s.routes(0) == [3, 4, 5] and not s.res["new_routes"][0].any()
    assert s.listener(0, "switches") == 5
    # listener 4 never hears itself, and its own order of arrival differs
    assert 4 not in s.routes(4) and sorted(s.routes(4)) == [-1, 3, 5]


def test_selection_order_is_hang_then_since_then_slot():
    s = Script(5, ForwardConfig(fanout=1, hang_hops=3))
    s.hop({3: "c"}, join_all(5, [0] * 5))
    assert s.routes(0) == [3]
    s.hop({3: "c", 1: "c"})                                  # equal SD_HANG: 3 has been active longer
    assert s.routes(0) == [3] and s.sender(3, "since") == 2 and s.sender(1, "since") == 1
    s.hop({1: "c"})                                          # 1 talks, 3 hangs over: SD_HANG decides
    assert s.routes(0) == [1] and s.res["new_routes"][0].tolist() == [1]
    s2 = Script(5, ForwardConfig(fanout=1))
    s2.hop({4: "c", 2: "c", 3: "c"}, join_all(5, [0] * 5))   # equal in everything: the lowest slot
    assert s2.routes(0) == [2] and s2.routes(2) == [3]


def test_sid_inside_the_hangover_is_forwarded_and_does_not_extend_it():
    s = Script(3, ForwardConfig(fanout=2, hang_hops=2))
    s.hop({1: "c"}, join_all(3, [0] * 3))
    s.hop({1: "s"})
    assert s.routes(0) == [1, -1] and s.row(0, 0) == s.sent[1, 0] and s.sender(1, "sids") == 1 and s.sender(1, "hang") == 2
    s.hop()
    assert s.routes(0) == [1, -1] and s.res["out_nbytes"][0].sum() == 0
    s.hop({1: "s"})                                          # hang_hops + 1 hops after its last codes packet: not active, not forwarded
    assert s.routes(0) == [-1, -1] and s.res["out_nbytes"][0].sum() == 0 and s.sender(1, "sids") == 2


def test_leave_and_join_free_routes():
    s = Script(4, ForwardConfig(fanout=3))
    s.hop({b: "c" for b in range(4)}, join_all(4, [0] * 4))
    assert s.routes(0) == [1, 2, 3]
    s.hop({b: "c" for b in range(4)}, [("leave", 2)])
    assert s.routes(0) == [1, -1, 3] and s.routes(2) == [-1, -1, -1] and not s.res["out_nbytes"][2].any()
    before = s.listener(1, "packets")
    s.hop({0: "c", 3: "c"}, [("join", 1, 0)])                # a new participant in an occupied slot: it is silent on this hop
    assert s.routes(0) == [-1, -1, 3] and s.routes(3) == [0, -1, -1]
    assert s.sender(1, "codes") == 0 and s.sender(1, "hang") == 0 and s.listener(1, "packets") == 2 < before
    assert s.routes(1) == [0, 3, -1] and s.res["new_routes"][1].tolist() == [1, 1, 0] and s.listener(1, "switches") == 2
    s.hop({1: "c", 3: "c"}, [("join", 1, 0)])                # joined and talking on the same hop: freed, then selected again
    assert s.routes(0) == [1, -1, 3] and s.res["new_routes"][0].tolist() == [1, 0, 0]
    s.hop({1: "c"}, [("join", 1, 0)])                        # the same index again: the owner did not change, so no flag
    assert s.routes(0) == [1, -1, 3] and not s.res["new_routes"][0].any()


def test_overflow_and_malformed_are_counted():
    s = Script(3, ForwardConfig(fanout=2, burst=2), m=2, n=4)
    s.hop({1: "cfsc", 2: "xx"}, join_all(3, [0] * 3))
    assert (s.sender(1, "codes"), s.sender(1, "sids"), s.sender(1, "overflow"), s.sender(1, "malformed")) == (3, 1, 2, 0)
    assert s.res["pick_count"].tolist() == [0, 2, 0] and s.res["pick"][1].tolist() == [0, 1] and s.res["pick"][2].tolist() == [-1, -1]
    assert s.row(0, 0, 0) == s.canon(1, 0) and s.row(0, 0, 1) == s.canon(1, 1) and wire.parse_transport(s.row(0, 0, 1), 11, 1, 4, 2, K_SID)[2]
    assert s.sender(2, "malformed") == 2 and s.sender(2, "hang") == 0 and s.routes(0) == [1, -1]
    s.hop({1: "xf"}, [("layers", 0, 1)])                     # the malformed arrival is not picked; layers 1 < m drops the redundant section
    assert s.res["pick"][1].tolist() == [1, -1] and s.sender(1, "malformed") == 1
    assert s.row(0, 0) == s.canon(1, 1, L=1) and len(s.row(0, 0)) == 3 + 2 and s.listener(0, "trimmed") == 1
    assert s.row(2, 0) == s.canon(1, 1) and s.listener(2, "trimmed") == 0


# ---------------------------------------------------------------- random traffic
RANDOM = dict(B=12, n=8, T=1, m=2, K=K_SID, rooms=3)
RANDOM_CFG = ForwardConfig(fanout=3, burst=2, hang_hops=3)


def run_random(hops, seed=21, p_event=0.2, **traffic_kw):
    """ForwardModel under Traffic: per hop (the result, the records, room, layers) and the final models"""
    r = RANDOM
    net = Traffic(r["B"], r["n"], r["T"], r["m"], r["K"], r["rooms"], seed, p_event=p_event, **traffic_kw)
    model, mem = ForwardModel(r["B"], RANDOM_CFG, r["n"], r["T"], r["m"], r["K"]), Membership(r["B"], r["n"])
    mem.apply(net.initial_events())
    steps = []
    for _ in range(hops):
        mem.apply(net.events())
        slots, packets, nbytes = net.hop()
        rec, offs = forward.arrival_records(slots, packets, nbytes, model.tb, r["B"])
        action = mem.action()
        steps.append((model.step_records(rec, offs, action, mem.room, mem.layers), rec, mem.room.copy(), mem.layers.copy(),
                      model.listener.state.copy(), action))
    return steps, model


def test_random_traffic_keeps_the_invariants():
    r = RANDOM
    steps, model = run_random(300)
    total = np.zeros((r["B"], 3), dtype=np.int64)
    prev_state = np.zeros_like(model.listener.state)
    for res, rec, room, layers, state, action in steps:
        counts = check_hop(res, rec, room, layers, RANDOM_CFG, r["n"], r["T"], r["m"], r["K"])
        base = np.where((action != 0)[:, None], 0, prev_state)                   # a join clears the row
        recount = np.concatenate([counts, res["new_routes"].sum(axis=1, keepdims=True)], axis=1)
        assert (forward.LR_PACKETS, forward.LR_BYTES, forward.LR_TRIMMED, forward.LR_SWITCHES) == (0, 1, 2, 3)
        assert np.array_equal(state - base, recount)
        prev_state = state
        total += counts
    sd = model.sender.state
    assert all(sd[:, i].sum() > 0 for i in range(forward.SD_WORDS)) and all(total[:, i].sum() > 0 for i in range(3))
    assert sum(int(res["new_routes"].sum()) for res, *_ in steps) > r["B"]


def test_rooms_are_independent():
    """other rooms' traffic replaced by different traffic and by garbage bytes: room 0's listener rows, routes and outputs are the same
    on every hop (the events are layer changes only, so the membership stays)"""
    r = RANDOM
    others = [b for b in range(r["B"]) if b % r["rooms"] != 0]
    base, _ = run_random(120, p_event=0.0)
    changed, _ = run_random(120, p_event=0.0, slot_seeds={b: 1000 + b for b in others}, garbage=others[::2])
    mine = [b for b in range(r["B"]) if b % r["rooms"] == 0]
    differs = False
    for (ra, _, _, _, sa, _), (rb, _, _, _, sb, _) in zip(base, changed):
        for key in ("out", "out_nbytes", "routes", "new_routes"):
            assert np.array_equal(ra[key][mine], rb[key][mine]), key
            differs = differs or not np.array_equal(ra[key][others], rb[key][others])
        assert np.array_equal(sa[mine], sb[mine])
    assert differs and sum(int(ra["out_nbytes"][mine].sum()) for ra, *_ in base) > 0
