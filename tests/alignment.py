"""Helpers of the pointer-alignment tests (tests/test_alignment_cpu.py, tests/test_gpu_alignment.py; the row table: tests/entry_rows.py).

`skew(t, k)`: a contiguous copy of `t` whose first element sits `4 * k` bytes behind a 16-byte boundary — what a caller gets from
`rec[:, :, k:k + T]` with B = 1, or from a cache kept as a view.  The references below are the plain definitions of the entry
points of `include/hilcodec_amd.h` in torch on the CPU, in whatever dtype their inputs have: float64 is the reference of the
sweep, float32 gives the reference's own rounding (the floor under every tolerance)."""
import torch
import torch.nn.functional as F


def skew_bytes(dtype: torch.dtype, k: int) -> int:
    """Byte offset of `skew(t, k)` behind a 16-byte boundary: 4 * k for the 4-byte types.  An 8-byte element cannot start on an odd
    multiple of 4 (no tensor can express it, and the kernels read such operands as 8-byte scalars): every k gives 8."""
    size = torch.empty((), dtype=dtype).element_size()
    if size <= 4:
        assert 4 % size == 0
        return 4 * k
    assert size == 8
    return 8


def skew(t: torch.Tensor, k: int) -> torch.Tensor:
    """copy of `t` (same shape, dtype, device, contiguous) in a fresh buffer of `numel + 16 bytes`, starting `skew_bytes` into it"""
    assert k in (1, 2, 3)
    size = t.element_size()
    off = skew_bytes(t.dtype, k)
    buf = torch.empty(t.numel() + 16 // size, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[off // size: off // size + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == off and v.shape == t.shape
    return v


# ---- plain references (dtype of the inputs) ---------------------------------------------------------------------------------------
def pro(x, scale, elu):
    v = x * scale
    return F.elu(v) if elu else v


def pw(a, wt, bias=None):
    """a [B,K,T], wt k-major [K,M] -> [B,M,T]"""
    return F.conv1d(a, wt.t().unsqueeze(-1).contiguous(), bias)


def dw(seq, w, bias, stride, To):
    """seq [B,C,L] = [cache | activated input]; w [C,k]; output o reads seq[o*stride : o*stride + k] (zeros past the end)"""
    C, k = w.shape
    need = (To - 1) * stride + k
    if need > seq.shape[2]:
        seq = F.pad(seq, (0, need - seq.shape[2]))
    return F.conv1d(seq, w.unsqueeze(1), bias, stride=stride, groups=C)[:, :, :To]


def with_hist(hist, a, pad):
    """[hist | a] along time; hist None = `pad` zeros"""
    if hist is None:
        hist = a.new_zeros(a.shape[0], a.shape[1], pad)
    return torch.cat([hist, a], dim=2)


def ref_pw_conv(x, wt, bias, res, in_scale, in_elu, out_scale):
    y = pw(pro(x, in_scale, in_elu), wt, bias) * out_scale
    return y if res is None else y + res


def ref_dw_conv(x, hist, w, bias, res, stride, in_scale, in_elu, out_scale, out_elu, raw_hist=False):
    k = w.shape[1]
    pad = k - stride
    To = (x.shape[2] + stride - 1) // stride
    if raw_hist and hist is not None:
        hist = pro(hist, in_scale, in_elu)
    seq = with_hist(None if hist is None else hist[:, :, hist.shape[2] - pad:], pro(x, in_scale, in_elu), pad)
    y = dw(seq, w, bias, stride, To) * out_scale
    if res is not None:
        y = y + res
    return (F.elu(y) if out_elu else y), seq[:, :, seq.shape[2] - pad:]


def ref_dw_convtr(x, hist, w, stride, in_scale, in_elu):
    """-> (y [B,C,T*r], new cache [B,C,1])"""
    B, C, T = x.shape
    cur = pro(x, in_scale, in_elu)
    first = cur.new_zeros(B, C, 1) if hist is None else hist.reshape(B, C, 1)
    prev = torch.cat([first, cur[:, :, :-1]], dim=2)
    y = w[:, :stride].view(1, C, 1, stride) * cur.unsqueeze(-1) + w[:, stride:].view(1, C, 1, stride) * prev.unsqueeze(-1)
    return y.reshape(B, C, T * stride), cur[:, :, -1:]


def ref_conv_post(x, hist, w, bias, in_scale, in_elu, out_scale, do_tanh):
    k = w.shape[1]
    seq = with_hist(hist, pro(x, in_scale, in_elu), k - 1)
    y = F.conv1d(seq, w.unsqueeze(0), bias) * out_scale
    return (torch.tanh(y) if do_tanh else y), seq[:, :, seq.shape[2] - (k - 1):]


def ref_dws(x, wt, dw_w, dw_b, hist, res, stride, in_scale, in_elu, out_scale, out_elu):
    """pointwise -> depthwise; -> (y, new cache = the last k - stride pointwise outputs of [hist | h])"""
    k = dw_w.shape[1]
    pad = k - stride
    h = pw(pro(x, in_scale, in_elu), wt)
    To = (x.shape[2] + stride - 1) // stride
    seq = with_hist(hist, h, pad)
    y = dw(seq, dw_w, dw_b, stride, To) * out_scale
    if res is not None:
        y = y + res
    return (F.elu(y) if out_elu else y), seq[:, :, seq.shape[2] - pad:]


def ref_up_conv(x, hist, tr_w, wt, bias, stride, in_scale, in_elu):
    u, cache = ref_dw_convtr(x, hist, tr_w, stride, in_scale, in_elu)
    return pw(u, wt, bias), cache


def ref_stft(wav, hist, basis_t, n_fft, hop, mean, std, normalize):
    """wav [B,1,T], hist [B,1,L] or None, basis_t [n_fft, m_pad] -> [B, n_fft/2+1, Tf]: the DFT as an explicit matrix product"""
    B, _, T = wav.shape
    left = wav.new_zeros(B, n_fft - 1) if hist is None else hist[:, 0, hist.shape[2] - (n_fft - 1):]
    fr = torch.cat([left, wav[:, 0]], dim=1).unfold(1, n_fft, hop)            # [B, Tf, n_fft]
    c = fr @ basis_t[:, :n_fft + 2]
    p = c[..., 0::2] ** 2 + c[..., 1::2] ** 2
    mag = p.clamp_min(1e-12).sqrt()
    if normalize == 2:
        out = mag
    else:
        out = mag.clamp_min(1e-5).log()
        if normalize == 1:
            out = (out - mean) / std
    return out.transpose(1, 2).contiguous()


def ref_spec_block(wav, hist, basis_t, wt, bias, x, n_fft, hop, mean, std, normalize, out_scale):
    y = pw(ref_stft(wav, hist, basis_t, n_fft, hop, mean, std, normalize), wt, bias) * out_scale
    return y if x is None else x + y


def ref_conv_pre(wav, hist, w, bias, in_scale):
    k = w.shape[1]
    seq = with_hist(None if hist is None else hist[:, :, hist.shape[2] - (k - 1):], wav, k - 1) * in_scale
    return F.conv1d(seq, w.unsqueeze(1), bias)


def ref_resblock(x, blk, hist):
    """blk = (w1 [C,C] k-major, dw1_w, dw1_b, w2, dw2_w, dw2_b, pre_scale, out_scale); hist = (hist1, hist2) or None
    -> (y, [new hist1, new hist2])"""
    w1, d1, b1, w2, d2, b2, pre, out = blk
    T = x.shape[2]
    s1 = with_hist(None if hist is None else hist[0], pw(pro(x, pre, True), w1), 4)
    m = F.elu(dw(s1, d1, b1, 1, T))
    s2 = with_hist(None if hist is None else hist[1], pw(m, w2), 4)
    y = x + dw(s2, d2, b2, 1, T) * out
    return y, [s1[:, :, T:], s2[:, :, T:]]


def ref_l2norm(x, eps, scale, channel_last_out):
    y = x / x.pow(2).sum(dim=1, keepdim=True).sqrt().clamp_min(eps) * scale
    return y.transpose(1, 2).contiguous() if channel_last_out else y


# ---- compositions for the chain and stage launches (the rows of tests/entry_rows.py, the families of tests/large_families.py) ------
def ref_blocks(a, x, streaming, out):
    for j, b in enumerate(a["blocks"]):
        x, new = ref_resblock(x, b, a["caches"][j] if streaming else None)
        if streaming:
            out[f"b{j}.hist1_out"], out[f"b{j}.hist2_out"] = new
    return x


def ref_encoder_stage(a, streaming, stage0, r, in_scale, N=64):
    """hilc_encoder_stage / hilc_encoder_stage0: [first conv + SpecBlock,] the blocks, the down-sampling layer"""
    out = {}
    if stage0:
        x = ref_conv_pre(a["wav"], a["whist"], a["pre_w"], a["pre_b"], 1 / 0.1122080159)
        x = ref_spec_block(a["wav"], a["whist"], a["basis_t"], a["swt"], a["sbias"], x, N, 1, -4.0, 2.8, 1, 0.37)
    else:
        x = a["x"]
    x = ref_blocks(a, x, streaming, out)
    y, h = ref_dws(x, a["wd"], a["ddw"], a["ddb"], a["dhist"], a["dres"], r, in_scale, True, 1.0, False)
    out["down.y"] = y
    if streaming:
        out["down.hist_out"] = h
    return out


def ref_decoder_stage(a, streaming, post, r):
    """hilc_decoder_stage / hilc_decoder_stage_post: the up-sampling layer, the blocks[, the closing conv]"""
    out = {}
    y, h = ref_up_conv(a["xin"], a["uhist"], a["tw"], a["wu"], a["bu"], r, 0.7071, True)
    if streaming:
        out["up.hist_out"] = h
    y = ref_blocks(a, y, streaming, out)
    if post:
        w, h = ref_conv_post(y, a["phist"], a["pw"], a["pb"], 0.5, True, 0.1122, True)
        out["post.wav"] = w
        if streaming:
            out["post.hist_out"] = h
    else:
        out["y"] = y
    return out
