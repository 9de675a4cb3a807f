"""The per-slot float entry points as cases (resampler, mixer, concealment gain, comfort noise, audio level, VBR: every operand class
S; the state-slot copies: class F, decided in the kernel) — shared by the alignment sweep and the red-zone tests (no tests here).

Each has its definition as a host model in hilcodec_amd/*.py, bit for bit.  `MISC` names every case and its operands; `CASES` holds
the built cases once `misc_run` has run."""
import numpy as np
import torch

from tests.alignment import skew
from tests.entry_rows import SENT


def misc_cases(dev):
    """name -> (operands {name: CPU tensor}, written operand names, fn(ops, t) -> {returned: tensor}, expected {name: CPU tensor})"""
    from hilcodec_amd import audio_level, dtx, mixer, vbr, wire
    from hilcodec_amd.resample import design, device_taps, reference
    cases = {}
    g = torch.Generator().manual_seed(1)
    # polyphase resampler, 16 kHz -> 24 kHz, a ragged hop with a history
    sp = design(16000, 24000)
    t = {"x": torch.rand(2, 1, 37, generator=g) * 2 - 1, "hist": torch.randn(2, 1, sp.Q - 1, generator=g) * 0.5, "hist_out": torch.full((2, 1, sp.Q - 1), SENT),
         "taps": device_taps(sp, dev).cpu()}
    y, h = reference(t["x"], sp, t["hist"])
    cases["resample_poly"] = (t, ("hist_out",), lambda ops, t: {"y": ops.resample_poly(t["x"], t["taps"], sp.L, sp.M, hist=t["hist"], hist_out=t["hist_out"])},
                              {"y": y, "hist_out": h})
    # mixer: levels, then rooms
    B, L = 6, 70
    rng = np.random.default_rng(7)
    wav = rng.uniform(-0.9, 0.9, (B, 1, L)).astype(np.float32)
    prev = rng.random(B) * np.array([1.0, 0.0, 1e4, 1.0, 1.0, 0.5])
    action = np.array([0, 0, 1, 0, 0, 0], dtype=np.int32)
    model = mixer.MixModel(B, mixer.MixConfig(1))
    model.score = torch.from_numpy(prev.copy())
    model.step(wav, [-1] * B, action)
    t = {"wav": torch.from_numpy(wav), "score": torch.from_numpy(prev.copy()), "action": torch.from_numpy(action)}
    cases["mix_levels"] = (t, ("score",), lambda ops, t: ops.mix_levels(t["wav"], t["score"], t["action"]) or {}, {"score": model.score.clone()})
    room = np.array([0, 0, 0, 1, -1, 1])
    score = rng.choice(np.array([0.0, 0.25, 1.0, 4.0]), B)
    speakers = mixer.select(room, score, 3)
    t = {"wav": torch.from_numpy(wav), "room": torch.from_numpy(room.astype(np.int32)), "score": torch.from_numpy(score),
         "mixed": torch.full((B, 1, L), SENT), "speakers": torch.full((B,), -9, dtype=torch.int32)}
    cases["mix_rooms"] = (t, ("mixed", "speakers"), lambda ops, t: ops.mix_rooms(t["wav"], t["room"], t["score"], 3, t["mixed"], t["speakers"]) or {},
                          {"mixed": torch.from_numpy(mixer.mix(wav.reshape(B, L), room, speakers)).view(B, 1, L), "speakers": torch.from_numpy(speakers)})
    # concealment gain: every ramp word of a 4-hop fade, an idle row and one out of range
    F, S = 4, 320
    G, W = wire.conceal_tables(F, S)
    ramp = torch.tensor([0, F + 1] + list(range(-F, 0)) + list(range(1, F + 1)), dtype=torch.int32)
    cw = torch.randn(len(ramp), 1, S, generator=g)
    exp = cw.clone()
    for b, r in enumerate(ramp.tolist()):
        if r != 0 and abs(r) <= F:
            a, c = (r - 1, r) if r > 0 else (-r, 0)
            exp[b] = cw[b] * (G[a] + (G[c] - G[a]) * W)              # fp32, one rounding per operation
    t = {"wav": cw, "ramp": ramp, "gains": G, "weights": W}
    cases["conceal_gain"] = (t, ("wav",), lambda ops, t: ops.conceal_gain(t["wav"], t["ramp"], t["gains"], t["weights"]) or {}, {"wav": exp})
    # comfort noise: a SID in every slot's row, then what dtx.cng_model makes of it
    K, T, B = 10, 1, 5
    stride = max(wire.packet_bytes(8, T), 1 + K)
    packets = torch.randint(0, 256, (B, stride), generator=g, dtype=torch.uint8)
    packets[:, 0] = torch.randint(0, 100, (B,), generator=g, dtype=torch.uint8)
    hold = torch.full((B,), 2, dtype=torch.int32)
    hold[3] = 0
    state = torch.zeros(B, dtx.state_words(K), dtype=torch.int32)
    e_state, e_hold, e_restore, noise = dtx.cng_model(state, packets, hold, None, K, T)
    t = {"packets": packets, "hold": hold, "state": state, "wav": torch.full((B, 1, 320 * T), 7.0), "gains": torch.from_numpy(dtx.gain_table()),
         "restore": torch.full((B,), 5, dtype=torch.int32)}
    cases["cng_synth"] = (t, ("hold", "state", "wav", "restore"),
                          lambda ops, t, K=K: ops.cng_synth(t["packets"], t["hold"], t["state"], t["wav"], t["gains"], K, None, t["restore"]) or {},
                          {"hold": e_hold, "state": e_state, "restore": e_restore,
                           "wav": torch.where(e_restore.bool()[:, None], noise, torch.full((B, 320 * T), 7.0)).view(B, 1, 320 * T)})
    # audio level of a hop
    x = (torch.rand(5, 1, 320, generator=g) * 2 - 1) * torch.tensor([1.0, 0.1, 1e-3, 0.0, 0.5]).view(5, 1, 1)
    t = {"x": x, "thr": torch.from_numpy(dtx.level_table()), "hold": torch.tensor([0, 0, 0, 0, 1], dtype=torch.int32), "level": torch.full((5,), -9, dtype=torch.int32)}
    want = audio_level.hop_level(x.numpy()).copy()
    want[4] = 127
    cases["audio_level"] = (t, ("level",), lambda ops, t: (ops.audio_level(t["x"], t["thr"], t["level"], t["hold"]), {})[1], {"level": torch.from_numpy(want.astype(np.int32))})
    # quality-targeted bitrate: vbr.VbrModel
    B, T, n, C, K = 5, 3, 8, 128, 1024
    cb = torch.randn(n + 1, K, C, generator=g) * 0.05
    cfg = vbr.VbrConfig(0.01, n_min=2)
    z = torch.randn(B, T, C, generator=g)
    idx = torch.randint(0, K, (n, B, T), generator=g)
    n_b = torch.randint(1, n + 1, (B,), generator=g, dtype=torch.int32)
    e_n, e_D, e_idx = vbr.VbrModel(B, cfg, n, T).step(z, idx, cb, n_b, None, None)
    t = {"z": z, "indices": idx.clone(), "codebooks": cb, "n_clip": n_b}

    def vbr_fn(ops, t):
        n_eff, D = ops.vbr_select(t["z"], t["indices"], t["codebooks"], min(n, vbr.floor_stages(cfg, 0)), cfg.rho, *vbr.bucket_bits(cfg, T, 0), t["n_clip"])
        return {"n_eff": n_eff, "distortion": D}
    cases["vbr_select"] = (t, ("indices",), vbr_fn, {"n_eff": e_n, "distortion": e_D, "indices": e_idx})
    # the state-slot entry points: `move` (csrc/state.hip) copies a piece as f32x4 words where both addresses are 16-byte aligned and its length
    # is a multiple of 4, word by word otherwise — decided per piece in the kernel.  Slices of 32, 15 and 16 floats per stream: in an aligned
    # block both forms occur, in a skewed one only the second; the result is a copy either way.
    from hilcodec_amd.ops import StateLayout
    B = 5
    layout = StateLayout([(B, 8, 4), (B, 3, 5), (B, 1, 16)], 1)
    block = torch.randn(layout.total, generator=g)
    records = torch.randn(3, layout.record_len, generator=g)
    action = torch.tensor([0, -1, 2, 1, 3], dtype=torch.int32)

    def part(k, b):
        return slice(layout.off[k] + b * layout.lens[k], layout.off[k] + (b + 1) * layout.lens[k])
    rec_off = [sum(layout.lens[:k]) for k in range(len(layout.lens))]
    want = block.clone()
    for k in range(len(layout.lens)):
        for b, a in enumerate(action.tolist()):
            if a == -1:
                want[part(k, b)] = 0
            elif a >= 1:
                want[part(k, b)] = records[a - 1, rec_off[k]: rec_off[k] + layout.lens[k]]
    t = {"block": block, "action": action, "records": records}
    cases["state_slots_apply"] = (t, ("block",), lambda ops, t: ops.state_slots_apply(t["block"], layout, t["action"], t["records"]) or {}, {"block": want})
    slots = torch.tensor([4, 0, 2], dtype=torch.int32)
    rec = torch.stack([torch.cat([block[part(k, b)] for k in range(len(layout.lens))]) for b in slots.tolist()])
    cases["state_slots_gather"] = ({"block": block, "slots": slots}, (), lambda ops, t: {"records": ops.state_slots_gather(t["block"], layout, t["slots"])},
                                   {"records": rec})
    dst = torch.randn(layout.total, generator=g)
    hold = torch.tensor([0, 1, 0, 2, 0], dtype=torch.int32)
    want = dst.clone()
    for k in range(len(layout.lens)):
        for b, h in enumerate(hold.tolist()):
            if h:
                want[part(k, b)] = block[part(k, b)]
    wav = torch.randn(B, 1, 37, generator=g)
    want_wav = wav.clone()
    want_wav[hold != 0] = 0
    t = {"src": block, "dst": dst, "hold": hold, "wav": wav}
    cases["state_slots_hold"] = (t, ("dst", "wav"), lambda ops, t: ops.state_slots_hold(t["src"], t["dst"], layout, t["hold"], wav=t["wav"]) or {},
                                 {"dst": want, "wav": want_wav})
    return cases


MISC = {"resample_poly": ("x", "hist", "hist_out", "taps"), "mix_levels": ("wav", "score", "action"),
        "mix_rooms": ("wav", "room", "score", "mixed", "speakers"), "conceal_gain": ("wav", "ramp", "gains", "weights"),
        "cng_synth": ("packets", "hold", "state", "wav", "gains", "restore"), "audio_level": ("x", "thr", "hold", "level"),
        "vbr_select": ("z", "indices", "codebooks", "n_clip"), "state_slots_apply": ("block", "action", "records"),
        "state_slots_gather": ("block", "slots"), "state_slots_hold": ("src", "dst", "hold", "wav")}
CASES = {}


def misc_run(e, name, operand=None, k=0):
    if not CASES:
        CASES.update(misc_cases(e.dev))
    t0, writes, fn, expected = CASES[name]
    assert tuple(t0) == MISC[name]
    t = {o: v.clone().to(e.dev) for o, v in t0.items()}
    if operand is not None:
        t[operand] = skew(t[operand], k)
    got = dict(fn(e.ops, t))
    torch.cuda.synchronize()
    for o, v in t0.items():
        if o not in writes:
            assert torch.equal(t[o].cpu(), v), f"{name}: the call changed its input `{o}`"
    got.update({o: t[o] for o in writes})
    return {o: v.cpu() for o, v in got.items()}, expected
