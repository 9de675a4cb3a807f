"""CPU: the oracle against the REAL reference modules' outputs, stored in tests/golden/vs_reference.npz by
`python oracle/make_golden.py --vs-reference`.  Different seeds and shapes than the other goldens, so the restatement is
pinned on more than one point.  Small outputs are stored whole; codebooks and streaming caches, too large to store, as
sha256 fingerprints of their bytes (bit-exact like torch.equal)."""
import hashlib
import json

import numpy as np
import pytest
import torch

from hilcodec_amd import synth
from oracle import hilcodec_oracle as O


def sha(t) -> str:
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def ref(golden):
    g = golden("vs_reference")
    g["meta"] = json.loads(str(g.pop("meta_json")))
    return g


def test_state_dict_keys_and_shapes(ref):
    for name in ("hil_speech", "hil_music"):
        mk = synth.model_kwargs(name)
        want = {k: tuple(s) for k, s in ref["meta"]["state_dict_shapes"][name]}
        got = synth.offline_param_shapes(mk)
        assert list(got.keys()) == [k for k, _ in ref["meta"]["state_dict_shapes"][name]]
        assert got == want
        assert ref["meta"]["n_params"][name] == 9577019          # scripts/PESQ STOI.ipynb:72-73


def test_model_kwargs_match_yaml(ref):
    for name in ("hil_speech", "hil_music"):        # configs/hilcodec_speech.yaml, configs/hilcodec_music.yaml
        assert ref["meta"]["yaml_model_kwargs"][name] == synth.model_kwargs(name)


@pytest.mark.parametrize("name,seed,T", [("hil_speech", 3, 6400), ("hil_music", 5, 3333)])
def test_offline_bit_exact(ref, name, seed, T):
    mk = synth.model_kwargs(name)
    sd = synth.synth_state_dict(name, seed=seed)
    x = synth.synth_clips(2, T, seed=seed * 11)
    with torch.no_grad():
        wav_o, nr_o, loss_o, aux = O.codec_forward(sd, x, mk)
    p = f"offline_{name}_"
    assert torch.equal(aux["z"], torch.from_numpy(ref[p + "z"]))
    assert torch.equal(aux["indices"], torch.from_numpy(ref[p + "indices"].astype(np.int64)))
    assert torch.equal(wav_o, torch.from_numpy(ref[p + "wav"]))
    assert torch.equal(loss_o, torch.from_numpy(ref[p + "loss"])) and (np.asarray(nr_o) == ref[p + "num_replaces"]).all()


def test_streaming_bit_exact_and_decoder_deviations(ref):
    mk = synth.model_kwargs("hil_speech")
    sd = synth.synth_state_dict("hil_speech", seed=13)
    p = O.stream_prepare(sd, mk)
    x = synth.synth_clips(2, 1600, seed=77)
    oe, od = O.stream_init_cache(mk, 2)
    assert [list(c.shape) for c in oe] == ref["meta"]["stream_cache_shapes"]["enc"]
    assert [list(c.shape) for c in od] == ref["meta"]["stream_cache_shapes"]["dec"]
    with torch.no_grad():
        for j, h in enumerate(range(0, 1600, 320)):
            xin = x[:, :, h:h + 320]
            zo, oe = O.stream_encoder(p, mk, xin, oe)
            io = O.stream_quantize(p, zo, 8)
            wo, od = O.stream_decoder(p, mk, O.stream_dequantize(p, io, 8), od)
            assert torch.equal(zo, torch.from_numpy(ref["stream_z"][j]))
            assert torch.equal(io, torch.from_numpy(ref["stream_indices"][j].astype(np.int64)))
            assert torch.equal(wo, torch.from_numpy(ref["stream_wav"][j]))
            assert [sha(c) for c in oe] == ref["meta"]["stream_cache_sha"][j]["enc"]
            assert [sha(c) for c in od] == ref["meta"]["stream_cache_sha"][j]["dec"]
        # the reference's streaming decoder is NOT its offline decoder
        z = O.encoder_forward(sd, x, mk)
        q, _, _, _ = O.rvq_forward(sd, z, 8, 8)
        _, od0 = O.stream_init_cache(mk, 2)
        w_stream, _ = O.stream_decoder(p, mk, q.transpose(1, 2), od0)
        assert (O.decoder_forward(sd, q, mk) - w_stream).abs().max() > 1e-2
        assert (O.decoder_forward(sd, q, mk, streaming_variant=True) - w_stream).abs().max() < 5e-6


def test_legacy_rvq_module(ref):
    D, K, nq = 128, 1024, 4
    sd = {}
    for i in range(nq):
        sd[f"quantizer.layers.{i}.embed"] = torch.from_numpy(synth.normalish(500 + i, K * D) * np.float32(0.3)).view(K, D)
    z = torch.from_numpy(synth.normalish(9, 3 * D * 20)).view(3, D, 20)
    with torch.no_grad():
        qo, nro, losso, _ = O.rvq_forward(sd, z, 3, nq, variant="legacy")
    assert torch.equal(torch.from_numpy(ref["legacy_q"]), qo)
    assert torch.allclose(torch.from_numpy(ref["legacy_loss"]), losso) and (ref["legacy_num_replaces"] == np.asarray(nro)).all()


def _check_state(ref, key, step, st, nq=3):
    """the oracle's training state after `step` against the reference's buffers: ema_num whole, the tables by fingerprint"""
    fp = ref["meta"][key + "_sha"][step]
    for i in range(nq):
        assert torch.equal(torch.from_numpy(ref[key + "_ema_num"][step, i]), st[f"layers.{i}.ema_num"])
        assert sha(st[f"layers.{i}.embed"]) == fp["embed"][i]
        assert sha(st[f"layers.{i}.ema_embed"]) == fp["ema_embed"][i]


def test_rvq_training_branch(ref):
    """oracle.rvq_train_step vs the reference ResidualVQ in train mode (n < Nq, expiry threshold on: the masks of
    expired codes must agree; the reference then replaces them with random batch vectors)."""
    D, K, nq, decay, init = 128, 1024, 3, 0.9, 0.5
    st = {}
    for i in range(nq):
        e = torch.from_numpy(synth.normalish(800 + i, K * D) * np.float32(0.3)).view(K, D)
        st[f"layers.{i}.embed"] = e.clone()
        st[f"layers.{i}.ema_embed"] = e * init
        st[f"layers.{i}.ema_num"] = torch.ones(K) * init
    for step in range(3):
        z = torch.from_numpy(synth.normalish(70 + step, 2 * D * 40)).view(2, D, 40)
        qo, losso, idxo, expired = O.rvq_train_step(st, z, 2, nq, decay, ema_num_threshold=0.46)
        assert torch.equal(torch.from_numpy(ref["train_indices"][step].astype(np.int64)), idxo)
        assert torch.equal(torch.from_numpy(ref["train_q"][step]), qo) and float(ref["train_loss"][step]) == float(losso)
        _check_state(ref, "train", step, st)
        assert expired.shape == (2, K)
        for i in range(2):
            assert torch.equal(expired[i], torch.from_numpy(ref["train_ema_num"][step, i]) < 0.46)
    assert expired.any()          # after three steps at decay 0.9 unused codes have dropped below 0.46


@pytest.mark.parametrize("threshold", [0.0, 0.46])
def test_legacy_rvq_training_branch(ref, threshold):
    """oracle.legacy_rvq_train_step vs the reference's older ResidualVQ in train mode: Laplace-smoothed division
    without an expiry threshold, plain division + expiry masks with one."""
    D, K, nq, decay, init = 128, 1024, 3, 0.9, 0.5
    st = {}
    for i in range(nq):
        e = torch.from_numpy(synth.normalish(820 + i, K * D) * np.float32(0.3)).view(K, D)
        st[f"layers.{i}.embed"] = e.clone()
        st[f"layers.{i}.ema_embed"] = e * init
        st[f"layers.{i}.ema_num"] = torch.ones(K) * init
    for step in range(3):
        z = torch.from_numpy(synth.normalish(75 + step, 2 * D * 40)).view(2, D, 40)
        # the reference runs without a threshold (its replacement vectors are random); the oracle's division rule
        # follows `threshold`, so the smoothed form is compared at 0.0 and only the masks at 0.46
        if threshold != 0.0:
            _, _, expired = O.legacy_rvq_train_step({k: v.clone() for k, v in st.items()}, z, 2, nq, decay,
                                                    ema_num_threshold=threshold)
            for i in range(2):
                assert torch.equal(expired[i], torch.from_numpy(ref["legacy_train_ema_num"][step, i]) < 0.46)
        # the oracle's state stays in lock-step with the reference's buffers (the 0.0 rule is the reference's own update)
        qo, losso, _ = O.legacy_rvq_train_step(st, z, 2, nq, decay, ema_num_threshold=0.0)
        assert torch.equal(torch.from_numpy(ref["legacy_train_q"][step]), qo)
        assert float(ref["legacy_train_loss"][step]) == float(losso)
        _check_state(ref, "legacy_train", step, st)
