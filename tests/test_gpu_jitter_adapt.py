"""GPU: adaptive playout of the receiver's jitter buffer (GraphedDecodeHop(jitter=JitterConfig(..., adapt=AdaptConfig(...)))).
hilc_jitter_adapt_step against jitter.JitterModel on traffic with drift, bursts and restarts; the adaptive receiver against a receiver
without a jitter buffer driven by step(...) from the model's decisions; the headed sender through a drifting network into an adaptive
and a fixed receiver — every comparison bit for bit (torch.equal / np.array_equal)."""
import numpy as np
import pytest
import torch

from hilcodec_amd import jitter, synth, wire
from hilcodec_amd.jitter import AdaptConfig, JitterConfig, JitterModel
from tests.hops import Network, arrival_records

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
HOP = 320
ADAPT = AdaptConfig(window=8, resync=3, force_windows=2)     # every branch fires within 150 hops


@pytest.fixture(scope="module")
def speech():
    return synth.streaming_model()


# ---------------------------------------------------------------- the kernel against jitter.py
KERNEL_CASES = [
    # (n, T, m, K, conceal, C, D, hops, seed): B = 70, a last workgroup with two idle waves
    (8, 1, 0, None, False, 4, 1, 150, 1),
    (8, 1, 2, 8, True, 8, 2, 150, 1),
    (8, 2, 2, None, True, 32, 5, 150, 1),
    (8, 3, 0, 8, False, 8, 0, 150, 1),
    (24, 7, 8, 8, True, 8, 2, 150, 1),                       # 280-byte rows, 70 words: the second pass of the lane loop
]
B_KERNEL = 70


def kernel_traffic(case):
    n, T, m, K, conceal, C, D, hops, seed = case
    cfg = JitterConfig(depth=D, capacity=C, adapt=ADAPT)
    model = JitterModel(B_KERNEL, cfg, n, m, T, K, conceal)
    net = Network(B_KERNEL, n, m, K, T, seed=seed, loss=0.06, delay=C + 2, dup=0.03, bad=0.02, hold=0.02, start=0.004,
                  sid=0.05 if K is not None else 0.0, restart=0.004)
    net.h[:6] = 65530                                        # these cross the 16-bit wrap early
    return cfg, model, net


def counters_cover(model, m, K):
    """every STAT_* and AD_* counter the configuration can move is non-zero somewhere in the batch"""
    st, ad = model.state, model.adapt
    missing = [name for i, name in enumerate(jitter.STAT_NAMES) if st[:, jitter.STAT_ACCEPTED + i].sum() == 0
               and not (name == "fec" and m == 0) and not (name == "noise" and K is None)]
    missing += [name for i, name in enumerate(jitter.AD_NAMES) if ad[:, jitter.AD_GROWN + i].sum() == 0]
    return missing


@pytest.mark.parametrize("case", KERNEL_CASES, ids=lambda c: "n{}-T{}-m{}-K{}-conceal{}-C{}-D{}".format(*c[:7]))
def test_jitter_adapt_step_kernel(case):
    from hilcodec_amd import ops
    n, T, m, K, conceal, C, D, hops, seed = case
    B = B_KERNEL
    cfg, model, net = kernel_traffic(case)
    stride = wire.packet_bytes(n + m, T)
    rw = (stride + 3) // 4
    assert (rw > 64) == (T == 7)
    state = torch.zeros(B, jitter.ST_WORDS, dtype=torch.int32, device=DEV)
    adapt = torch.zeros(B, jitter.AD_WORDS, dtype=torch.int32, device=DEV)
    meta = torch.zeros(B, C, dtype=torch.int32, device=DEV)
    ring = torch.zeros(B, C, rw, dtype=torch.int32, device=DEV)
    rows = torch.zeros(3, B, dtype=torch.int32, device=DEV)
    pk = torch.zeros(B, stride, dtype=torch.uint8, device=DEV)
    max_a = 4 * B
    for k in range(hops):
        slots, packets, nbytes, action, hold = net.hop()
        assert len(slots) <= max_a
        arr, offs = arrival_records(slots, packets, nbytes, net.tbytes, B, max_a)
        hold_d = torch.from_numpy(hold).to(DEV)
        rows.fill_(-9)
        pk.fill_(0xEE)
        ops.jitter_adapt_step(arr, offs, hold_d, rows[0], pk, state, meta, ring, adapt, n, m, T, K, cfg,
                              action=torch.from_numpy(action).to(DEV), lost=rows[1] if conceal else None, fec=rows[2] if m else None)
        want = model.step(action, hold, slots, packets, nbytes)
        assert np.array_equal(hold_d.cpu().numpy(), want["hold"]), k
        assert np.array_equal(rows[0].cpu().numpy(), want["n"]), k
        if conceal:
            assert np.array_equal(rows[1].cpu().numpy(), want["lost"]), k
        if m:
            assert np.array_equal(rows[2].cpu().numpy(), want["fec"]), k
        assert np.array_equal(pk.cpu().numpy(), want["packets"]), k
        assert np.array_equal(state.cpu().numpy(), model.state), k
        assert np.array_equal(adapt.cpu().numpy(), model.adapt), k
        assert np.array_equal(meta.cpu().numpy(), model.meta), k
        got_ring = ring.cpu().numpy().view(np.uint8).reshape(B, C, 4 * rw)
        assert np.array_equal(got_ring[:, :, :stride], model.body) and not got_ring[:, :, stride:].any(), k
    assert counters_cover(model, m, K) == []


# ---------------------------------------------------------------- play() against the explicit step()
def explicit_step(rx, rows):
    """drive a receiver without jitter with the model's decisions"""
    hv = rows["hold"]
    return rx.step(torch.from_numpy(rows["packets"]), rows["n"].tolist(), hold=np.nonzero(hv == 1)[0].tolist(),
                   lost=np.nonzero(rows["lost"])[0].tolist(), fec=np.nonzero(rows["fec"])[0].tolist(),
                   sid=np.nonzero(hv == 2)[0].tolist(), silent=np.nonzero(hv == 3)[0].tolist())


def compare(a, b, k):
    for x, y in zip(a.cache_dec, b.cache_dec):
        assert torch.equal(x, y), k
    assert torch.equal(a.concealed, b.concealed), k
    assert torch.equal(a.cng_state, b.cng_state), k


RX = dict(sessions=True, conceal=True, fec_stages=2, cng_order=8)


def test_adaptive_play_matches_explicit_step(speech):
    from hilcodec_amd.graph_step import GraphedDecodeHop
    B, n, m, K, hops = 6, 8, 2, 8, 80
    cfg = JitterConfig(2, 8, adapt=ADAPT)
    jx = GraphedDecodeHop(speech, B, 1, n, DEV, jitter=cfg, **RX)
    ex = GraphedDecodeHop(speech, B, 1, n, DEV, **RX)
    model = JitterModel(B, cfg, n, m, 1, K, True)
    net = Network(B, n, m, K, 1, seed=4, loss=0.08, delay=6, dup=0.02, bad=0.02, hold=0.03, sid=0.06, restart=0.01, every=10)
    for k in range(hops):
        slots, packets, nbytes, action, hold = net.hop()
        if k == 50:
            assert model.adapt[2].any()
            action[2] = 1                                    # a start in the middle clears the slot's adapt row
        for b in np.nonzero(action)[0]:
            jx.start(int(b))
            ex.start(int(b))
        rows = model.step(action, hold, slots, packets, nbytes)
        a = jx.play(slots, torch.from_numpy(packets), nbytes, hold=np.nonzero(hold)[0].tolist()).clone()
        b = explicit_step(ex, rows).clone()
        assert torch.equal(a, b), k
        compare(jx, ex, k)
        assert np.array_equal(jx.jitter_state.cpu().numpy(), model.state), k
        assert np.array_equal(jx.jitter_adapt.cpu().numpy(), model.adapt), k
        if k == 50:
            assert not model.adapt[2, jitter.AD_GROWN:].any() and not jx.jitter_adapt[2, jitter.AD_GROWN:].any()
    ad = model.adapt
    assert ad[:, jitter.AD_GROWN].sum() > 0 and ad[:, jitter.AD_SHRUNK].sum() > 0
    # a start with no arrival on that hop: the whole row is zero
    jx.start(3)
    jx.play([], torch.zeros(0, jx.tstride, dtype=torch.uint8), [])
    assert not jx.jitter_adapt[3].any() and not jx.jitter_state[3].any() and jx.jitter_adapt.any()


def test_jitter_adapt_accessor(speech):
    from hilcodec_amd.graph_step import GraphedDecodeHop
    fixed = GraphedDecodeHop(speech, 2, 1, 8, DEV, sessions=True, jitter=JitterConfig(2, 8))
    with pytest.raises(RuntimeError):
        fixed.jitter_adapt
    plain = GraphedDecodeHop(speech, 2, 1, 8, DEV, sessions=True)
    with pytest.raises(RuntimeError):
        plain.jitter_adapt
    ad = GraphedDecodeHop(speech, 2, 1, 8, DEV, sessions=True, jitter=JitterConfig(2, 8, adapt=AdaptConfig()))
    assert ad.jitter_adapt.shape == (2, jitter.AD_WORDS) and ad.jitter_adapt.dtype == torch.int32


# ---------------------------------------------------------------- end to end: the headed sender through a drifting network
@pytest.mark.parametrize("trace", ["slow", "restart"])
def test_sender_to_adaptive_and_fixed_receiver(speech, trace):
    """slow: the receiver runs 21 hops for every 20 of the sender's (on every 20th of its hops the sender does not step);
    restart: the sender starts again at hop 150, the receivers are not told"""
    from hilcodec_amd.graph_step import GraphedDecodeHop, GraphedEncodeHop
    B, n, m, hops = 4, 8, 2, 300
    tx = GraphedEncodeHop(speech, B, HOP, n, DEV, sessions=True, fec_stages=m, header=True)
    cfgs = {"adaptive": JitterConfig(2, 8, adapt=AdaptConfig()), "fixed": JitterConfig(2, 8)}
    rx = {name: GraphedDecodeHop(speech, B, 1, n, DEV, jitter=cfg, **RX) for name, cfg in cfgs.items()}
    ex = {name: GraphedDecodeHop(speech, B, 1, n, DEV, **RX) for name in cfgs}
    models = {name: JitterModel(B, cfg, n, m, 1, 8, True) for name, cfg in cfgs.items()}
    x = (torch.randn(B, hops * HOP, generator=torch.Generator().manual_seed(9)) * 0.1).to(DEV)
    sent = 0
    action = np.ones(B, dtype=np.int32)
    none = np.zeros(B, dtype=np.int32)
    for k in range(hops):
        if trace == "restart" and k == 150:
            for b in range(B):
                tx.start(b)
        if trace == "slow" and k % 20 == 19:
            slots, packets, nbytes = [], np.zeros((0, rx["fixed"].tstride), dtype=np.uint8), []
        else:
            pk, nb = tx.step(x[:, sent * HOP:(sent + 1) * HOP].reshape(B, 1, HOP))
            sent += 1
            slots, packets, nbytes = list(range(B)), pk.cpu().numpy(), nb.cpu().numpy().tolist()
            assert min(nbytes) > 3
        for name in cfgs:
            rows = models[name].step(action, none, slots, packets, nbytes)
            a = rx[name].play(slots, torch.from_numpy(packets), nbytes).clone()
            b = explicit_step(ex[name], rows).clone()
            assert torch.equal(a, b), (name, k)
            assert np.array_equal(rx[name].jitter_state.cpu().numpy(), models[name].state), (name, k)
        assert np.array_equal(rx["adaptive"].jitter_adapt.cpu().numpy(), models["adaptive"].adapt), k
        action[:] = 0
    ad, fx = rx["adaptive"].jitter_state.cpu().numpy(), rx["fixed"].jitter_state.cpu().numpy()
    adapt = rx["adaptive"].jitter_adapt.cpu().numpy()
    # the adaptive receiver's decoded count stays within the model's; the fixed receiver piles up LATE
    assert np.array_equal(ad[:, jitter.STAT_DECODED], models["adaptive"].state[:, jitter.STAT_DECODED])
    if trace == "slow":
        # a hop the sender skips costs at most one late packet and one lost hop (the window of 50 hops is longer than the 20 between
        # two skips, so most of them are followed through the urgent debt); what was not late is decoded, but for the D + 1 in the ring
        drifts = hops // 20
        assert (ad[:, jitter.STAT_LATE] <= drifts).all() and (ad[:, jitter.STAT_LOST] <= drifts).all()
        assert (ad[:, jitter.STAT_DECODED] >= sent - drifts - 3).all() and (adapt[:, jitter.AD_FORCED] == 0).all()
        assert (fx[:, jitter.STAT_LATE] >= 200).all()
    else:
        assert (adapt[:, jitter.AD_RESYNC] == 1).all() and (ad[:, jitter.STAT_LATE] <= AdaptConfig().resync).all()
        assert (fx[:, jitter.STAT_LATE] == hops - 150).all()
