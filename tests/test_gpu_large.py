"""Every entry point of the hot path on activation tensors just below and at 4 GiB ("Large tensors").

One row of `tests/large.py: CASES` is one entry point and form; it runs at two sizes of its governing tensor — the largest
activation the launch reads or writes, or for a streaming form the product its launch path guards: "below", the largest legal
shape under 2^32 bytes, and "at", the smallest legal shape from 2^32 bytes on — and, one per family, with B = 3 clips of just over
2 GiB each, so that the clip bases lie beyond 2^31 and 2^32 bytes.  Operands are periodic in time and cycle through three patterns
over the clips (tests/large.py; tests/large_families.py builds each family's operands, call, reference and fall-back), so a float64
reference of three periods on the CPU covers the whole output; the compare runs over EVERY element on the device.  Per case:

  1. the call returns HILC_OK, or refuses (HILC_ERR_UNSUPPORTED / HILC_ERR_SHAPE): then every caller-owned output still holds its
     sentinel, a small launch of the same entry succeeds afterwards, the `hilcodec_amd.ops` mirror declines the shape too, and the
     launches the engine falls back to (public `ops` wrappers) give the result within the tolerance;
  2. on success every output — caches included — is within the tolerance of the row of tests/entry_rows.py named by the case
     (no new number), finite, and clips with the same pattern are bit-identical (three patterns: that binds the streaming rows, whose tens
     of thousands of clips repeat the cycle; three clips are three patterns, so there a clip read from another clip's base shows as an error);
  3. the common prefix of the "below" and the "at" output agrees: bit for bit where both ran a form that promises the same fmaf
     chains — a refused streaming form against its fall-back included — and within the tolerance for hilc_conv_post, whose header promises
     no more.

"below" asserts through the entry's `*_supported` query, the `ops` mirror or the launch-path predicate that the fast form is the one
that runs.  For hilc_pw_conv, hilc_dws_conv and hilc_up_conv the library has no query: the predicate is a transcription of `lin_ok`
(tests/large.py), so the `form=` a case prints is derived from the shape, not reported by the launch; that both cores give the same
bits is what the below / at comparison observes.  One-channel waveform tensors as the GOVERNING tensor are left out (the inputs of conv_pre and the resampler, the mixer's
rows): 4 GiB of mono fp32 is 12 hours of audio.  The last test runs one clip of 466 s through the whole model."""
import time
import types

import pytest
import torch

from hilcodec_amd import synth
from tests import large as L
from tests.entry_rows import ROWS, SENT, env  # noqa: F401  (env: the fixture)
from tests.large_families import FAMILIES, references

pytestmark = pytest.mark.gpu

_KEEP = {}          # case -> the periodic outputs of its "below" run, kept on the device until the "at" run has compared them


# ======================================================================================================================
# the runner
# ======================================================================================================================
def gpu_sentinel(t):
    return bool((t == (SENT if t.is_floating_point() else int(SENT))).all())


def launch(e, f, outs=None):
    """one call of the family's entry with fresh sentinel outputs -> (rc, {output: device tensor})"""
    o = f.o
    if outs is None:
        outs = {k: torch.full(shape, SENT if dtype.is_floating_point else int(SENT), dtype=dtype, device=e.dev) for k, (shape, dtype) in o.outs.items()}
    p = {k: (None if t is None else t.data_ptr()) for k, t in list(o.ins.items()) + list(outs.items())}
    assert all(v is None or v % 16 == 0 for v in p.values())
    rc = f.call(p)
    torch.cuda.synchronize()
    return rc, outs


def check_outputs(c, f, outs, ref, tol, what):
    o = f.o
    for name, want in ref.items():
        y = outs[name]
        assert not gpu_sentinel(y[:1]), f"{c.name} [{what}]: output `{name}` was not written"
        if name in o.rates:
            P = o._n(o.P, o.rates[name])
            got = L.compare_periodic(y, want, P)
        else:          # a cache: one value per clip, row and tap
            got = L.compare_periodic(y, want, want.shape[2])
        bar = 0.0 if y.dtype == torch.int64 else tol
        print(f"{c.name} [{what}] {name} {tuple(y.shape)}: max |y - ref64| = {got.err:.3e} at clip {got.clip} row {got.row} t {got.t} "
              f"(byte offset {got.byte_offset}), tolerance {bar:.1e}")
        assert got.finite, f"{c.name} [{what}] `{name}`: not finite at clip {got.clip} row {got.row} t {got.t} (byte offset {got.byte_offset})"
        assert got.err <= bar, (f"{c.name} [{what}] `{name}`: {got.err:.3e} > {bar:.1e} at clip {got.clip} row {got.row} t {got.t} "
                                f"(byte offset {got.byte_offset})")
        assert L.identical_clips_equal(y), f"{c.name} [{what}] `{name}`: two clips with the same pattern differ"
    assert set(ref) == set(outs), (set(ref), set(outs))


def prefix_agrees(c, name, below, at, rate, exact, tol):
    """the common prefix of the two sizes' outputs: the clips both have, and of each the outputs whose window lies inside the shorter clip"""
    Bc = min(below.shape[0], at.shape[0])
    n = min(int(c.sizes["below"]["T"] * rate), int(c.sizes["at"]["T"] * rate), below.shape[2], at.shape[2])
    worst, same = 0.0, True
    per = max(1, L.CHUNK_BYTES // max(1, below.shape[1] * n * 4))
    tc = max(1, min(n, L.CHUNK_BYTES // (below.shape[1] * 4)))
    for b0 in range(0, Bc, per):
        for t0 in range(0, n, tc):
            u, v = below[b0:b0 + per, :, t0:min(n, t0 + tc)], at[b0:min(Bc, b0 + per), :, t0:min(n, t0 + tc)]
            if exact:
                same = same and torch.equal(u, v)
            else:
                worst = max(worst, float((u.double() - v.double()).abs().max()))
    print(f"{c.name} below vs at `{name}`: common prefix {Bc} x {below.shape[1]} x {n}: " + (f"bit-identical = {same}" if exact else f"max diff {worst:.3e}"))
    assert same, f"{c.name} `{name}`: the results just below and at 4 GiB differ in their common prefix"
    assert worst <= tol, f"{c.name} `{name}`: the results just below and at 4 GiB differ by {worst:.3e} > {tol:.1e}"


def run_case(e, c, size, keep=False):
    """-> {periodic output: device tensor} of a successful run (or of the fall-back behind a refusal), and whether the entry ran"""
    d = c.sizes[size]
    need, (free, _) = L.need_bytes(c, size), torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f"{c.name} [{size}] needs {need / 2 ** 30:.1f} GiB of device memory, {free / 2 ** 30:.1f} GiB are free")
    tol = ROWS[c.tolrow].tol
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    f = FAMILIES[c.family](e, c, d)
    gov = L.governing_bytes(c, d)
    fast, form = f.fast()
    if size == "below":
        assert gov < L.LIMIT and fast, f"{c.name} [below]: the fast form does not take this shape"
    ref, floor = references(f)
    assert tol >= 4 * floor, f"{c.name}: tolerance {tol:.1e} is below 4 x the reference's own rounding {floor:.2e}"
    rc, outs = launch(e, f)
    if rc == 0:
        check_outputs(c, f, outs, ref, tol, size)
        ran = True
    else:
        # a refusal: clean, nothing written, the device healthy, the mirror declines as well, the fall-back is right
        assert rc in (-4, -1), f"{c.name} [{size}]: return code {rc}"
        assert size != "below", f"{c.name} [below]: refused with {rc}"
        for name, t in outs.items():
            assert gpu_sentinel(t), f"{c.name} [{size}]: refused with {rc}, but output `{name}` was written"
        del outs
        assert f.mirror() is False, f"{c.name} [{size}]: the entry refuses ({rc}) what its hilcodec_amd.ops mirror accepts"
        small = FAMILIES[c.family](e, c, dict(d, B=4))
        rc2, outs2 = launch(e, small)
        assert rc2 == 0, f"{c.name}: a small launch after the refusal failed with {rc2}"
        check_outputs(c, small, outs2, references(small)[0], tol, "small launch after the refusal")
        del small, outs2
        outs = f.fallback()
        assert outs is not None, f"{c.name} [{size}]: refused with {rc} and no fall-back is known"
        torch.cuda.synchronize()
        check_outputs(c, f, outs, ref, tol, size + ", fall-back")
        form, ran = f"refused ({rc}); fall-back: pointwise + depthwise launches", False
    kept = {k: v for k, v in outs.items() if k in f.o.rates}
    rates = dict(f.o.rates)
    del f, outs
    torch.cuda.synchronize()
    print(f"LARGE case={c.name} size={size} governing_bytes={gov} rc={rc} form=\"{form}\" seconds={time.time() - t0:.2f} "
          f"peak_gib={torch.cuda.max_memory_allocated() / 2 ** 30:.2f} need_gib={need / 2 ** 30:.1f}")
    return kept, rates, ran


def release():
    """free the case's tensors; a device that reports an error ends the session — no later case runs on it"""
    import gc
    gc.collect()
    try:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    except RuntimeError as err:
        pytest.exit(f"the device reports `{err}`: no further large-tensor case runs on it", returncode=3)


def ids():
    return [(name, size) for name, c in L.CASES.items() for size in c.sizes]


@pytest.mark.parametrize("name,size", ids(), ids=[f"{n}-{s}" for n, s in ids()])
def test_entry_point_at_the_offset_limit(env, name, size):
    c = L.CASES[name]
    try:
        if size == "at":
            below = _KEEP.pop(name, None)
            if below is None:          # run alone: its own "below" first
                below = run_case(env, c, "below")
            at, rates, ran = run_case(env, c, "at")
            # (a refused streaming form against its fall-back too: measured bit-identical, and the engine's hop must not change its bits
            # with the batch size)
            exact = bool(c.exact and ROWS[c.tolrow].exact is True and below[2])
            for k, y in at.items():
                prefix_agrees(c, k, below[0][k], y, rates[k], exact, ROWS[c.tolrow].tol)
            del below, at
        else:
            got = run_case(env, c, size)
            if size == "below":
                _KEEP.clear()          # (whatever an earlier row left behind: its "at" case did not run)
                _KEEP[name] = got
            del got
    finally:
        if size != "below":
            _KEEP.clear()
        release()


def test_every_row_of_the_issue_is_in_the_table():
    fams = {c.family for c in L.CASES.values()}
    assert fams == set(FAMILIES)
    assert all(c.tolrow in ROWS for c in L.CASES.values())
    assert sum(1 for c in L.CASES.values() if c.stream_guard is not None) == 7 and sum(1 for c in L.CASES.values() if "b3" in c.sizes) >= 10


# ======================================================================================================================
# the long clip through the model
# ======================================================================================================================
@pytest.fixture(scope="module")
def long_clip():
    """the model, and the oracle on three periods of the long clip's input"""
    from oracle import hilcodec_oracle as O
    from tests.models import build
    model, mk, _ = build("hil_speech")
    sd = synth.synth_state_dict("hil_speech", seed=7)
    assert L.model_receptive_field(mk) < L.MODEL_P // 2 and L.MODEL_P % 320 == 0 and L.wraps_visible(L.MODEL_P)
    pat = L.model_pattern()
    with torch.no_grad():
        wav_o, _, _, aux = O.codec_forward(sd, pat.repeat(1, 1, 3), mk)
    gaps = O.rvq_gaps_fp64(sd, aux["z"], aux["indices"])
    return types.SimpleNamespace(model=model, mk=mk, pat=pat, z=aux["z"], idx=aux["indices"], wav=wav_o, gaps=gaps)


@pytest.mark.parametrize("T", [L.MODEL_T_BELOW, L.MODEL_T_AT], ids=["one-chunk-below", "at-4GiB"])
def test_long_clip_through_the_model(long_clip, T):
    """One clip of 466 s — the smallest whose decoder activation [1, 96, T] reaches 4 GiB (the engine cannot chunk one clip) — and the
    next shorter one: every period of z, of the indices and of the decoded waveform after the first against the oracle's third period, at
    the offline bars of the suite (|dz| < 1e-5, |dwav| < 1e-4; an index may differ only on a float64 near-tie < 1e-4, at most one phase)."""
    from hilcodec_amd import engine, ops
    g, dev = long_clip, torch.device("cuda:0")
    free = torch.cuda.mem_get_info()[0]
    if free < (12 << 30):          # measured peak: 6.2 GiB
        pytest.skip(f"the long clip needs 12 GiB of device memory, {free / 2 ** 30:.1f} GiB are free")
    # the decoder's last stage writes [1, 96, T]: the largest activation of the clip (engine._decoder_clip_elems, tests/test_large_cpu.py)
    assert (96 * T * 4 >= L.LIMIT) == (T == L.MODEL_T_AT) and 96 * L.MODEL_T_BELOW * 4 < L.LIMIT and engine._clip_chunks(1, 96 * T) == [(0, 1)]
    # what runs (the engine's own predicates): every decoder stage is a fused offline stage launch — the last two whole, the closing conv in
    # the last — and they alone touch the clip's 4 GiB tensors, the [1, 192, T / 2] between the last two stages and the [1, 96, T] that never
    # leaves the last launch; every other launch, the whole encoder included, sees less than 4 GiB and keeps the linear cores
    ds, es, Fr = g.model.decoder.plan(dev), g.model.encoder.plan(dev), T // 320
    assert engine.FUSE_RESBLOCK and engine.FUSE_UPSAMPLE and engine._decoder_clip_elems(ds, Fr) == 96 * T
    assert engine._encoder_clip_elems(es, T) * 4 < L.LIMIT
    t, big = Fr, []
    for st in ds.stages:
        c = st.pw_wt.shape[1]
        nb = engine._stage_fusable_blocks(st, torch.empty(1, 2 * c, t, device="meta"), False)
        t *= st.ratio
        assert nb >= 1 and ops.decoder_stage_supported(c, t, nb, st.ratio, 1, streaming=False), (c, t, nb)
        if c * t * 4 >= L.LIMIT or 2 * c * (t // st.ratio) * 4 >= L.LIMIT:
            assert nb == len(st.blocks), (c, t, nb)
            big.append(c)
    assert ops.decoder_stage_post_supported(96, T, 3, 2, ds.post_w.shape[1]) and big == ([192, 96] if T == L.MODEL_T_AT else [])
    P, Fp = L.MODEL_P, L.MODEL_P // 320
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    x = L.periodic(g.pat, T, 1, dev)
    with torch.no_grad():
        z = g.model.encoder(x)
        q, _, _, idx = g.model.quantizer(z, None, return_indices=True)
        wav = g.model.decoder(q)
    torch.cuda.synchronize()
    assert z.shape == (1, 128, T // 320) and wav.shape == (1, 1, T) and torch.isfinite(wav).all()
    dz = L.compare_periodic(z, g.z.double(), Fp)
    print(f"long clip T={T}: |dz| = {dz.err:.3e} at frame {dz.t} row {dz.row}")
    assert dz.finite and dz.err < 1e-5
    di = L.compare_periodic(idx, g.idx.double(), Fp)
    flips = 0
    if di.err > 0:          # a differing argmin: the same phase in every period (asserted), excused only as a float64 near-tie
        nper = (T // 320) // Fp
        first = idx[0, :, :3 * Fp].cpu()
        bad = (first != g.idx[0]).any(dim=0).nonzero().flatten().tolist()
        phases = sorted({t % Fp for t in bad if t >= Fp})
        for t in bad:
            s0 = int((first[:, t] != g.idx[0, :, t]).nonzero()[0])
            assert g.gaps[0, s0, t] < 1e-4, f"genuine index mismatch at frame {t} stage {s0}: gap {g.gaps[0, s0, t]:.3e}"
        later = idx[0, :, Fp:]          # every frame behind period 0, the clip's last, partial period included, repeats period 1
        assert torch.equal(later, idx[0, :, Fp:2 * Fp].repeat(1, nper)[:, :later.shape[1]]), "the indices are not periodic"
        flips = len(phases) + sum(1 for t in bad if t < Fp and t % Fp not in phases)
    assert flips <= 1, f"{flips} near-tie flips"
    if flips == 0:
        dw0 = L.compare_periodic(wav, g.wav.double(), P)
        print(f"long clip T={T}: |dwav| (own codes) = {dw0.err:.3e} at sample {dw0.t}")
        assert dw0.finite and dw0.err < 1e-4
    # the decoder on the reference's own codes: the oracle's indices of periods 0 and 1, then its third period for every later one
    cb = g.model.quantizer.spec(dev).codebooks
    idx_ref = g.idx[:, :, L.ref_index(0, T // 320, Fp, True)].contiguous().to(dev)
    q_ref = ops.rvq_decode(idx_ref, cb, g.idx.shape[1], channel_last=False, stage_major=False)
    del q, wav
    with torch.no_grad():
        wav2 = g.model.decoder(q_ref)
    dw = L.compare_periodic(wav2, g.wav.double(), P)
    print(f"long clip T={T}: |dwav| (reference codes) = {dw.err:.3e} at sample {dw.t}; seconds={time.time() - t0:.1f} "
          f"peak_gib={torch.cuda.max_memory_allocated() / 2 ** 30:.2f}")
    assert dw.finite and dw.err < 1e-4
    del x, z, idx, wav2, q_ref
    release()
