"""Every entry point of the hot path on 4-byte-aligned views: fall back or refuse ("Pointer alignment").

One row per entry point and shape: the `BASE` rows of tests/entry_rows.py, which holds the table and what runs a row.  A row builds
its operands on the device, calls the C ABI with raw pointers, and has a plain float64 reference on the CPU (tests/alignment.py).
The call runs once with every operand 16-byte aligned, then once per operand and k = 1, 2, 3 with only that operand moved 4 * k
bytes off (`skew`).  The row's table gives the audited class of every operand:

  S / F  the call succeeds, is within the op's tolerance of the float64 reference and — caches and every other output included —
         `torch.equal` to the aligned call (the fall-backs promise the same fmaf chains);
  R      the call is refused (RuntimeError out of `check`), every caller-owned output still holds its sentinel, and the device
         is healthy afterwards.

The tolerance of a row is the one the op's own test in tests/test_gpu_ops.py uses; it may not be below 4 x the rounding of the
reference itself (float32 against float64 on the CPU, the `FLOORS` table as measured, asserted again at run time).
Copyable R operands are tested a second time through `hilcodec_amd.ops`, where the wrapper copies them: equal to the aligned call."""
import pytest
import torch

from hilcodec_amd import synth
from tests.alignment import skew
from tests.entry_rows import BASE, BLK, FLOORS, KS, ROWS, SENT, aligned, built, check_ok, env, raw_blocks, rnd, run, sentinel  # noqa: F401  (env: the fixture)
from tests.slot_cases import CASES, MISC, misc_run

pytestmark = pytest.mark.gpu


def test_every_operand_has_a_class(env):
    assert set(FLOORS) == set(ROWS)
    for name, r in ROWS.items():
        assert r.tol >= 4 * FLOORS[name], name
        b = built(env, name)
        assert set(r.cls) == {o for o, t in b.ins.items() if t is not None} | set(b.outs), name
        assert set(r.cls.values()) <= {"S", "F", "R"}, name


@pytest.mark.parametrize("name", BASE)
def test_aligned_call(env, name):
    aligned(env, name)


@pytest.mark.parametrize("name,operand", [(n, o) for n in BASE for o in ROWS[n].cls])
def test_one_operand_skewed(env, name, operand):
    e, r = env, ROWS[name]
    base = aligned(e, name)
    for k in KS:
        rc, outs = run(e, name, operand, k)
        what = f"{operand} + {4 * k} B"
        if r.cls[operand] == "R":
            assert rc == -4, f"{name} [{what}]: expected HILC_ERR_UNSUPPORTED, got {rc}"
            with pytest.raises(RuntimeError):
                e.L.check(rc, name)
            for o, t in outs.items():
                assert sentinel(t), f"{name} [{what}]: the refused call wrote `{o}`"
            torch.cuda.synchronize()
            continue
        assert rc == 0, f"{name} [{what}]: class {r.cls[operand]} but the call returned {rc}"
        check_ok(e, name, outs, what)
        for o, t in outs.items():
            if r.exact is True or o in r.exact:
                assert torch.equal(t, base[o]), f"{name} [{what}]: `{o}` differs from the aligned call by {float((t.double() - base[o].double()).abs().max()):.3e}"


def test_rvq_encode_sums_its_own_indices(env):
    """the RVQ rows have no float64 reference of their arg-min (a near-tie may legitimately flip); what they return must be consistent:
    q = the float64 sum of the code vectors of the returned indices, frame_err = |z - q|^2"""
    for name in ("rvq_encode-valu-2x128x9", "rvq_encode-mfma-8x128x1024"):
        outs, a = aligned(env, name), built(env, name).aux
        idx, cb = outs["indices"], a["codebooks"].double()
        assert int(idx.min()) >= 0 and int(idx.max()) < cb.shape[1]
        q = sum(cb[s][idx[:, s]] for s in range(idx.shape[1])).transpose(1, 2)
        assert float((outs["q"].double() - q).abs().max()) <= 1e-6
        err = (a["z"].double() - q).pow(2).sum(1).reshape(-1)
        assert float((outs["frame_err"].double() - err).abs().max()) <= 1e-5 * float(err.max())
        # and the indices are the float64 arg-min wherever float64 sees a clear winner
        res = a["z"].double().transpose(1, 2).reshape(-1, cb.shape[2])
        for s in range(idx.shape[1]):
            d = cb[s].pow(2).sum(-1)[None] - 2 * res @ cb[s].t()
            best2 = d.topk(2, dim=1, largest=False)
            got = idx[:, s].reshape(-1)
            clear = (best2.values[:, 1] - best2.values[:, 0]) > 1e-4
            assert torch.equal(got[clear], best2.indices[:, 0][clear]), (name, s)
            res = res - cb[s][got]


# ======================================================================================================================
# the model layer copies what the library would refuse
# ======================================================================================================================
def _ops_cases(e):
    """(name, fn(t) -> outputs, {operand: aligned tensor}) — `fn` calls hilcodec_amd.ops with the operands of the dict, one case per
    wrapper that copies (`_al16`), streaming and offline; packed tables are held in the dict, so they are what gets skewed"""
    ops, dev = e.ops, e.dev
    cases = []

    def add(name, fn, t):
        cases.append((name, fn, t))

    def D(t):
        return t.to(dev)
    B, K, M, T = 2, 17, 64, 132
    t = {"x": D(rnd(1, B, K, T)), "wt": D(rnd(2, K, M) / K ** 0.5), "res": D(rnd(3, B, M, T))}
    add("pw_conv", lambda t: (ops.pw_conv(t["x"], t["wt"], None, res=t["res"], in_scale=0.8, in_elu=True),), t)
    B, K, M, T = 2, 33, 96, 36
    t = {"x": D(rnd(1, B, K, T)), "wt": D(rnd(2, K, M) / K ** 0.5), "dw_w": D(rnd(3, M, 5) * 0.5), "dw_b": D(rnd(4, M) * 0.1), "res": D(rnd(5, B, M, T))}
    add("dws_conv-k5", lambda t: (ops.dws_conv(t["x"], t["wt"], t["dw_w"], t["dw_b"], res=t["res"], in_scale=0.86, in_elu=True, out_scale=0.37),), t)
    t = {"x": D(rnd(1, 2, 16, 64)), "wt": D(rnd(2, 16, 32) / 4), "dw_w": D(rnd(3, 32, 8) * 0.5), "dw_b": D(rnd(4, 32) * 0.1)}
    add("dws_conv-r4", lambda t: (ops.dws_conv(t["x"], t["wt"], t["dw_w"], t["dw_b"], stride=4, in_scale=0.86, in_elu=True),), t)
    for name, (B, K, M, T, k, r) in (("dws_conv_stream-long", (3, 16, 32, 160, 8, 4)), ("dws_conv_stream-r5", (5, 16, 32, 40, 10, 5)),
                                     ("dws_conv_stream-k5", (5, 32, 32, 8, 5, 1))):
        t = {"x": D(rnd(1, B, K, T)), "wt": D(rnd(2, K, M) / K ** 0.5), "dw_w": D(rnd(3, M, k) * 0.5), "dw_b": D(rnd(4, M)), "hist": D(rnd(5, B, M, k - r))}
        add(name, lambda t, r=r: ops.dws_conv_stream(t["x"], t["wt"], t["dw_w"], t["dw_b"], t["hist"], stride=r, in_elu=True), t)
    # the up-sampling stage: offline r = 2, a hop with its cache r = 4, the expanded table r = 5
    for name, (B, K, M, Tin, r, stream) in (("up_conv-r2", (2, 32, 16, 6, 2, False)), ("up_conv-r4-stream", (2, 32, 16, 4, 4, True)),
                                            ("up_conv-r5-expanded-stream", (2, 48, 24, 4, 5, True))):
        t = {"x": D(rnd(100 + K, B, K, Tin)), "tr_w": D(rnd(80, K, 2 * r) * 0.3), "wt": D(rnd(81, K, M) / K ** 0.5), "bias": D(rnd(82, M) * 0.1)}
        if r == 5:
            t["taps"] = ops.up_conv_taps(t["tr_w"], r)
        if stream:
            t["hist"] = D(rnd(30, B, K, 1) * 0.6)
        add(name, lambda t, r=r, stream=stream: tuple(ops.up_conv(t["x"], t["tr_w"], t["wt"], t["bias"], r, in_scale=0.7071, hist=t.get("hist"),
                                                                  want_hist=True, taps=t.get("taps"))) if stream
            else (ops.up_conv(t["x"], t["tr_w"], t["wt"], t["bias"], r, in_scale=0.7071),), t)
    t = {"wav": D(synth.synth_clips(2, 64, seed=1)), "basis_t": D(e.fold.stft_basis_layout(synth.stft_basis(16)))}
    add("stft_logmag", lambda t: (ops.stft_logmag(t["wav"], t["basis_t"], 16, 1, normalize=2),), t)
    # hilc_conv_post's generic kernel sums the channels in another order (the sweep's one exception): ops copies, the bits stay
    t = {"x": D(rnd(9, 2, 24, 36)), "hist": D(rnd(8, 2, 24, 4) * 0.6), "w": D(rnd(3, 24, 5) / 20)}
    add("conv_post", lambda t: ops.conv_post(t["x"], t["w"], None, in_scale=0.707, hist=t["hist"], want_hist=True), t)
    N = 64
    dft_p, nyq, pw_p = ops.spec_block_tables(D(e.fold.stft_basis_layout(synth.stft_basis(N))), D(rnd(N + 1, N // 2 + 1, N) / 6), N)
    sp = {"wav": D(synth.synth_clips(2, 128, seed=2)), "whist": D(synth.synth_clips(2, N - 1, seed=3)), "dft": dft_p, "nyq": nyq, "pw": pw_p,
          "sbias": D(rnd(N + 2, N) * 0.1)}
    t = dict(sp, x=D(rnd(9, 2, N, 128)))
    add("spec_block", lambda t: (ops.spec_block(t["wav"], t["dft"], t["nyq"], t["pw"], t["sbias"], t["x"], N, 1, -4.0, 2.8, True, 0.37, hist=t["whist"]),), t)
    t = dict(sp, pre_w=D(rnd(71, N, 5) * 0.5), pre_b=D(rnd(72, N) * 0.1))
    add("spec_block_conv_pre", lambda t: (ops.spec_block_conv_pre(t["wav"], t["dft"], t["nyq"], t["pw"], t["sbias"], t["pre_w"], t["pre_b"], 1 / 0.1122080159,
                                                                  N, 1, -4.0, 2.8, True, 0.37, hist=t["whist"]),), t)

    # ---- the fused block, the chain and the stage ops, a hop with every cache and the offline form
    def block_dict(C, n, B, streaming, pack):
        raw = raw_blocks(C, n)
        t = {}
        for j, b in enumerate(raw):
            for nm, w in zip(BLK, b[:6]):
                t[f"b{j}.{nm}"] = pack(D(w)) if nm in ("w1t", "w2t") else D(w)
            if streaming:
                t[f"b{j}.hist1"], t[f"b{j}.hist2"] = D(rnd(7 + j, B, C, 4) * 0.7), D(rnd(8 + j, B, C, 4) * 0.7)
        return raw, t

    def blocks_of(t, raw, streaming):
        n = len(raw)
        return ([tuple(t[f"b{j}.{nm}"] for nm in BLK) + (raw[j][6], raw[j][7]) for j in range(n)],
                [[t[f"b{j}.hist1"], t[f"b{j}.hist2"]] for j in range(n)] if streaming else None)

    def flat(r):
        """(y, [caches], cache, ...) or y -> a flat list of tensors"""
        if torch.is_tensor(r):
            return [r]
        out = []
        for v in r:
            out.extend(flat(v))
        return out
    B = 3
    for streaming in (True, False):
        tag = "stream" if streaming else "offline"
        pack = lambda w, s=streaming: ops.resblock_chain_pack(w, s)          # noqa: E731
        # one block: the packed matrices are operands of the dict
        C, T = 64, 8
        raw, t = block_dict(C, 1, B, streaming, ops.resblock_pack)
        t["x"] = D(rnd(C, B, C, T))
        add(f"resblock-{tag}", lambda t, raw=raw, s=streaming: flat(ops.resblock(t["x"], *[t[f"b0.{nm}"] for nm in BLK], raw[0][6], raw[0][7],
                                                                          hist=[t["b0.hist1"], t["b0.hist2"]] if s else None)), t)
        raw, t = block_dict(C, 2, B, streaming, pack)
        t["x"] = D(rnd(C, B, C, T))
        add(f"resblock_chain-{tag}", lambda t, raw=raw, s=streaming: flat(ops.resblock_chain(t["x"], *blocks_of(t, raw, s))), t)
        # encoder stages: narrow (C = 128, r = 4: the taps are class S) and wide (C = 512, r = 8: class R)
        for C, r in ((128, 4), (512, 8)):
            raw, t = block_dict(C, 2, B, streaming, pack)
            wd = D(rnd(70, C, 2 * C) / C ** 0.5)
            t.update({"x": D(rnd(C + 1, B, C, T)), "w_lo": pack(wd[:, :C].contiguous()), "w_hi": pack(wd[:, C:].contiguous()),
                      "dw_w": D(rnd(73, 2 * C, 2 * r) * 0.3), "dw_b": D(rnd(74, 2 * C) * 0.1), "res": D(rnd(75, B, 2 * C, T // r) * 0.5)})
            if streaming:
                t["dhist"] = D(rnd(30, B, 2 * C, r) * 0.6)

            def enc(t, raw=raw, s=streaming, r=r):
                blocks, hist = blocks_of(t, raw, s)
                return flat(ops.encoder_stage(t["x"], blocks, (t["w_lo"], t["w_hi"], t["dw_w"], t["dw_b"], 0.77, r), hist=hist, down_hist=t.get("dhist"),
                                              res=t["res"]))
            add(f"encoder_stage-{C}-{tag}", enc, t)
        # the encoder's first stage with the first conv and its SpecBlock
        C, T0 = 64, 128 if streaming else 8
        raw, t = block_dict(C, 2, B, streaming, pack)
        wd = D(rnd(70, C, 2 * C) / C ** 0.5)
        t.update({"wav": D(synth.synth_clips(B, T0, seed=T0)), "dft": dft_p, "nyq": nyq, "pw": pw_p, "sbias": sp["sbias"], "pre_w": D(rnd(71, C, 5) * 0.5),
                  "pre_b": D(rnd(72, C) * 0.1), "w_lo": pack(wd[:, :C].contiguous()), "w_hi": pack(wd[:, C:].contiguous()),
                  "dw_w": D(rnd(73, 2 * C, 4) * 0.3), "dw_b": D(rnd(74, 2 * C) * 0.1), "res": D(rnd(75, B, 2 * C, T0 // 2) * 0.5)})
        if streaming:
            t["dhist"], t["whist"] = D(rnd(30, B, 2 * C, 2) * 0.6), D(synth.synth_clips(B, N - 1, seed=9))

        def enc0(t, raw=raw, s=streaming):
            blocks, hist = blocks_of(t, raw, s)
            spec = (t["dft"], t["nyq"], t["pw"], t["sbias"], t["pre_w"], t["pre_b"], 1 / 0.1122080159, -4.0, 2.8, True, 0.37)
            return flat(ops.encoder_stage0(t["wav"], spec, blocks, (t["w_lo"], t["w_hi"], t["dw_w"], t["dw_b"], 0.77, 2), res=t["res"], hist=hist,
                                           down_hist=t.get("dhist"), wav_hist=t.get("whist")))
        add(f"encoder_stage0-{tag}", enc0, t)
        # decoder stages: C = 96 / r = 2 and C = 384 / r = 5 (the expanded tap table), and the last stage with the closing conv
        for C, r, Tin, post in ((96, 2, 2, False), (384, 5, 4, False), (96, 2, 2, True)):
            raw, t = block_dict(C, 3, B, streaming, pack)
            tw, wu = D(rnd(80, 2 * C, 2 * r) * 0.3), D(rnd(81, 2 * C, C) / (2 * C) ** 0.5)
            taps = ops.up_conv_taps(tw, r)
            t.update({"xin": D(rnd(5, B, 2 * C, Tin)), "tr_w": tw if taps is None else taps, "w_lo": pack(wu[:C].contiguous()), "w_hi": pack(wu[C:].contiguous()),
                      "bias": D(rnd(82, C) * 0.1)})
            if streaming:
                t["uhist"] = D(rnd(30, B, 2 * C, 1) * 0.6)
            if post:
                t["post_w"], t["post_b"] = D(rnd(83, C, 5) * 0.2), D(rnd(84, 1) * 0.1)
                if streaming:
                    t["phist"] = D(rnd(31, B, C, 4) * 0.6)

            def dec(t, raw=raw, s=streaming, r=r, post=post):
                blocks, hist = blocks_of(t, raw, s)
                up = (t["tr_w"], t["w_lo"], t["w_hi"], t["bias"], 0.7071, r)
                if post:
                    return flat(ops.decoder_stage_post(t["xin"], up, blocks, (t["post_w"], t["post_b"], 0.5, 0.1122, True), hist, t.get("uhist"),
                                                       t.get("phist")))
                return flat(ops.decoder_stage(t["xin"], up, blocks, hist, t.get("uhist")))
            add(f"decoder_stage{'_post' if post else ''}-{C}-{tag}", dec, t)
    return cases


OPS_CASES = ["pw_conv", "dws_conv-k5", "dws_conv-r4", "dws_conv_stream-long", "dws_conv_stream-r5", "dws_conv_stream-k5", "up_conv-r2", "up_conv-r4-stream",
             "up_conv-r5-expanded-stream", "stft_logmag", "conv_post", "spec_block", "spec_block_conv_pre"] + [
    f"{n}-{tag}" for tag in ("stream", "offline") for n in ("resblock", "resblock_chain", "encoder_stage-128", "encoder_stage-512", "encoder_stage0",
                                                            "decoder_stage-96", "decoder_stage-384", "decoder_stage_post-96")]
_OPS_CASES = {}


@pytest.mark.parametrize("name", OPS_CASES)
def test_ops_copy_misaligned_inputs(env, name):
    """Through hilcodec_amd.ops no contiguous input raises: whatever the library would refuse is copied to a fresh allocation first, and the
    result — every cache included — is `torch.equal` to the call on aligned operands.  Every tensor operand of the wrapper is skewed in turn."""
    if not _OPS_CASES:
        _OPS_CASES.update({n: (fn, t) for n, fn, t in _ops_cases(env)})
        assert list(_OPS_CASES) == OPS_CASES
    fn, t = _OPS_CASES[name]
    assert all(v.data_ptr() % 16 == 0 for v in t.values())
    base = [o.clone() for o in fn(t)]
    for operand in t:
        for k in KS:
            got = fn({o: (skew(v, k) if o == operand else v) for o, v in t.items()})
            torch.cuda.synchronize()
            assert len(got) == len(base)
            for i, (a, b) in enumerate(zip(got, base)):
                assert torch.equal(a, b), f"ops.{name}: `{operand}` + {4 * k} B changes output {i} by {float((a - b).abs().max()):.3e}"


OUT_CASES = {"resblock-stream": ("hist_out", r"resblock: `hist2_out`"), "resblock_chain-stream": ("hist_out", r"resblock_chain: `hist_out\[3\]`"),
             "encoder_stage-128-stream": ("down_hist_out", r"encoder_stage: `dhist_out`"), "encoder_stage0-stream": ("down_hist_out", r"encoder_stage0: `dhist_out`"),
             "decoder_stage-96-stream": ("hist_out", r"decoder_stage: `hist_out\[5\]`"),
             "decoder_stage_post-96-stream": ("post_hist_out", r"decoder_stage_post: `post_hist_out`")}


@pytest.mark.parametrize("name", list(OUT_CASES))
def test_ops_name_the_misaligned_output(env, name):
    """A cache the caller owns as an output cannot be copied: a misaligned one that the kernel writes as 16-byte words raises before anything
    is launched, and the message names the wrapper, the operand and the 16-byte rule.  The same call with aligned outputs fills them."""
    ops, dev = env.ops, env.dev
    if not _OPS_CASES:
        _OPS_CASES.update({n: (fn, t) for n, fn, t in _ops_cases(env)})
    _, t = _OPS_CASES[name]
    kind, message = OUT_CASES[name]
    B = 3

    def call(last):
        """the wrapper with caller-owned outputs; `last` = the one named in the message"""
        def fresh(*shape):
            return torch.full(shape, SENT, device=dev)
        n = sum(1 for o in t if o.endswith(".w1t"))
        C = t["b0.dw1_b"].shape[0]
        raw = raw_blocks(C, n)
        blocks = [tuple(t[f"b{j}.{nm}"] for nm in BLK) + (raw[j][6], raw[j][7]) for j in range(n)]
        hist = [[t[f"b{j}.hist1"], t[f"b{j}.hist2"]] for j in range(n)]
        outs = [[fresh(B, C, 4), fresh(B, C, 4)] for _ in range(n)]
        if kind == "hist_out":
            outs[-1][1] = last(B, C, 4)
        owned = [o for pair in outs for o in pair]
        if name.startswith("resblock-"):
            ops.resblock(t["x"], *[t[f"b0.{nm}"] for nm in BLK], raw[0][6], raw[0][7], hist=hist[0], hist_out=outs[0])
        elif name.startswith("resblock_chain"):
            ops.resblock_chain(t["x"], blocks, hist, hist_out=outs)
        elif name.startswith("encoder_stage0"):
            owned.append(last(B, 2 * C, 2))
            spec = (t["dft"], t["nyq"], t["pw"], t["sbias"], t["pre_w"], t["pre_b"], 1 / 0.1122080159, -4.0, 2.8, True, 0.37)
            ops.encoder_stage0(t["wav"], spec, blocks, (t["w_lo"], t["w_hi"], t["dw_w"], t["dw_b"], 0.77, 2), res=t["res"], hist=hist, hist_out=outs,
                               down_hist=t["dhist"], down_hist_out=owned[-1], wav_hist=t["whist"])
        elif name.startswith("encoder_stage"):
            owned.append(last(B, 2 * C, 4))
            ops.encoder_stage(t["x"], blocks, (t["w_lo"], t["w_hi"], t["dw_w"], t["dw_b"], 0.77, 4), hist=hist, hist_out=outs, down_hist=t["dhist"],
                              down_hist_out=owned[-1], res=t["res"])
        elif name.startswith("decoder_stage_post"):
            owned.append(last(B, C, 4))
            ops.decoder_stage_post(t["xin"], (t["tr_w"], t["w_lo"], t["w_hi"], t["bias"], 0.7071, 2), blocks, (t["post_w"], t["post_b"], 0.5, 0.1122, True),
                                   hist, t["uhist"], t["phist"], hist_out=outs, post_hist_out=owned[-1])
        else:
            ops.decoder_stage(t["xin"], (t["tr_w"], t["w_lo"], t["w_hi"], t["bias"], 0.7071, 2), blocks, hist, t["uhist"], hist_out=outs)
        torch.cuda.synchronize()
        return owned
    for k in KS:
        made = []

        def skewed(*shape):
            made.append(skew(torch.full(shape, SENT, device=dev), k))
            return made[-1]
        with pytest.raises(RuntimeError, match=message + r".*16-byte"):
            call(skewed)
        torch.cuda.synchronize()
        assert len(made) == 1 and sentinel(made[0].cpu())
    owned = call(lambda *shape: torch.full(shape, SENT, device=dev))
    assert all(not sentinel(o.cpu()) for o in owned)


# ======================================================================================================================
# the per-slot float entry points (tests/slot_cases.py: resampler, mixer, concealment gain, comfort noise, audio level, VBR: every
# operand class S; the state-slot copies: class F, decided in the kernel).
# Each has its definition as a host model in hilcodec_amd/*.py, bit for bit; the aligned call must equal that definition and every
# call with one operand skewed — float32, float64, int32, int64 and uint8 rows alike — must equal the aligned call.
# ======================================================================================================================
@pytest.mark.parametrize("name,operand", [(n, o) for n, ops_ in MISC.items() for o in (None,) + ops_])
def test_per_slot_entry_points(env, name, operand):
    base, expected = misc_run(env, name)
    assert set(base) == set(expected)
    for o, want in expected.items():
        assert base[o].dtype == want.dtype and torch.equal(base[o], want), f"{name}: `{o}` differs from the host model"
    if operand is None:
        return
    for k in KS:
        got, _ = misc_run(env, name, operand, k)
        for o in base:
            assert torch.equal(got[o], base[o]), f"{name} [{operand} + {skew(CASES[name][0][operand], k).data_ptr() % 16} B]: `{o}` differs from the aligned call"


# ======================================================================================================================
# model level
# ======================================================================================================================
def _set_stage_launches(model, on):
    for half in (model.encoder, model.decoder):
        half.exec_options.stage_launches = on


@pytest.mark.parametrize("stage_launches", [True, False])
def test_offline_model_on_a_trimmed_recording(env, stage_launches):
    """One recording trimmed at the front, `rec[:, :, k:k + 1280]` with B = 1: contiguous, 4 * k bytes off, accepted by the model — indices
    and waveform equal the same call on a copy of the slice."""
    import hilcodec_amd
    m = hilcodec_amd.HILCodec(24000, 1, **synth.model_kwargs("hil_speech")).eval()
    m.load_state_dict(synth.synth_state_dict("hil_speech", seed=7), strict=False)
    for layer in m.quantizer.layers:
        layer.initted = True
    rec = synth.synth_clips(1, 1280 + 8, seed=11).to(env.dev)
    assert rec.data_ptr() % 16 == 0
    _set_stage_launches(m, stage_launches)
    try:
        with torch.no_grad():
            for k in KS:
                x = rec[:, :, k:k + 1280]
                assert x.is_contiguous() and x.data_ptr() % 16 == 4 * k
                outs = []
                for inp in (x.clone(), x):
                    z = m.encoder(inp)
                    q, _, _, idx = m.quantizer(z, None, return_indices=True)
                    outs.append((idx, m.decoder(q)))
                torch.cuda.synchronize()
                assert outs[0][0].shape[2] == 4 and outs[0][1].shape == (1, 1, 1280)
                assert torch.equal(outs[0][0], outs[1][0]), k
                assert torch.equal(outs[0][1], outs[1][1]), (k, float((outs[0][1] - outs[1][1]).abs().max()))
    finally:
        _set_stage_launches(m, True)


@pytest.mark.parametrize("stage_launches", [True, False])
def test_streaming_model_with_every_cache_a_misaligned_view(env, stage_launches):
    """The eager streaming model keeps the caches it is handed as views: B = 3, two hops, every cache tensor replaced by `skew(cache, 1)` —
    indices, waveform and all new caches equal the run on the aligned caches."""
    from tests.hops import build_streaming
    model, mk, sd = build_streaming(seed=11)
    B = 3
    x = synth.synth_clips(B, 640, seed=5).to(env.dev)
    _set_stage_launches(model, stage_launches)
    try:
        def two_hops(prepare):
            ce, cd = model.initialize_cache(x)
            out = []
            with torch.no_grad():
                for h in range(2):
                    ce, cd = [prepare(c) for c in ce], [prepare(c) for c in cd]
                    z, ce = model.encoder(x[:, :, 320 * h: 320 * (h + 1)], *ce)
                    idx = model.quantizer(z, 8)
                    w, cd = model.decoder(model.dequantizer(idx, 8), *cd)
                    out.append((idx, w, list(ce), list(cd)))
            torch.cuda.synchronize()
            return out

        def skewed(c):
            v = skew(c, 1)
            assert v.data_ptr() % 16 == 4
            return v
        base, got = two_hops(lambda c: c), two_hops(skewed)
        for h in range(2):
            assert torch.equal(base[h][0], got[h][0]), h
            assert torch.equal(base[h][1], got[h][1]), (h, float((base[h][1] - got[h][1]).abs().max()))
            for which in (2, 3):
                assert len(base[h][which]) == len(got[h][which])
                for i, (a, b) in enumerate(zip(base[h][which], got[h][which])):
                    assert torch.equal(a, b), (h, which, i)
    finally:
        _set_stage_launches(model, True)
